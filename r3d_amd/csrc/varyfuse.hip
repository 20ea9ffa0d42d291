// The activation-magnitude token fuser of model/futr_safuser_tokenfusion_vary.py, the seam between the two embeddings
// and the fuser block:
//   forward : exchanged_rgb[c] = alpha[c] * dep[c] on the selected RGB channels, exchanged_dep[c] = alpha[c] * rgb[c] on
//             the selected depth channels, every other channel passes through (:40-56; the selection itself, k = C // 4
//             smallest of mean_(B,T) |x|, is r3d_colabssum + r3d_token_select), embd_drop (:76),
//             fuser.blocks.0.norm1 (transformerblock.py:122).
//   backward: norm1 backward (+ the residual gradient) -> dropout -> adjoint of the scaled exchange -> d_rgb_pre (times
//             input_embed's ReLU gate), d_dep (into the depth LayerNorm + ReLU backward), and one [N, C] term matrix whose
//             column sum is d alpha.  The column sum is left to a fixed-order reduction (a row-sum job of the grouped
//             weight-gradient launch or r3d_rowmod_sum_batched): no atomics, bitwise the same from run to run.
// One workgroup (2 waves = the two modality tokens) per frame, as the BN-blend seam (bnfuse.hip).  norm1's forward tail and
// backward row are seam_rows.h's; here are the alpha-scaled exchange and its adjoint.
#include "common.h"
#include "../../include/r3d_hip.h"
#include "seam_rows.h"

namespace r3d {

struct VaryArgs {
    const float* rgb; const float* dep;                         // [N][C] embeddings (post ReLU)
    const float* alpha;                                         // [C]
    const float* m_rgb; const float* m_dep;                     // [C] 1 = selected channel
    const uint8_t* drop; float drop_scale; const float* ln1_g; const float* ln1_b;
    float* x0; float* h1; float* m1; float* r1;
    // backward only
    const float* d_h1; const float* add1;
    float* d_rgb_pre; float* d_dep; float* t_dal; float* ws_n1;
    int N, C;
};

template <int EPL>
__global__ __launch_bounds__(128) void vary_exchange_fwd_kernel(const VaryArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x & 63, t = threadIdx.x >> 6, C = a.C;
    const size_t rowo = (size_t)n * C, row = (size_t)2 * n + t;
    int cc[EPL];
    seam_cols<EPL>(lane, C, cc);
    float x[EPL], g1[EPL], b1[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        const float r = a.rgb[rowo + cc[e]], d = a.dep[rowo + cc[e]];
        const float own = t == 0 ? r : d, oth = t == 0 ? d : r;
        const float sel = (t == 0 ? a.m_rgb : a.m_dep)[cc[e]];
        const float keep = a.drop ? a.drop_scale * (float)a.drop[row * C + cc[e]] : 1.f;
        float v = (sel != 0.f ? a.alpha[cc[e]] * oth : own) * keep;
        if (c >= C) v = 0.f;
        x[e] = v;
        g1[e] = a.ln1_g[cc[e]]; b1[e] = a.ln1_b[cc[e]];
        if (c < C) a.x0[row * C + c] = v;
    }
    seam_norm1_fwd<EPL>(x, g1, b1, a.m1, a.r1, a.h1, row, lane, C);
}

template <int EPL>
__global__ __launch_bounds__(128) void vary_exchange_bwd_kernel(const VaryArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];        // G[2][C] | P[2][2][C]
    const int n = blockIdx.x, lane = threadIdx.x & 63, t = threadIdx.x >> 6, C = a.C;
    float* G = lds;
    float* P = lds + 2 * C;
    const size_t rowo = (size_t)n * C, row = (size_t)2 * n + t;
    int cc[EPL];
    seam_cols<EPL>(lane, C, cc);
    SeamRowBwd<EPL, false, false> tk;
    tk.load(a.d_h1, a.x0, a.m1, a.r1, a.ln1_g, a.add1, nullptr, a.drop, a.drop_scale, row, C, cc);
    tk.norm1_bwd(G, P, t, lane, C, cc);
    __syncthreads();
    if (t == 1) {
        if (!a.ws_n1) return;                       // (the fuser chain's backward already left these partials)
        seam_norm1_partials<EPL>(P, a.ws_n1, n, lane, C);
        return;
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        if (c >= C) continue;
        const float g0 = G[c], g1v = G[C + c];                 // gradients of exchanged_rgb / exchanged_dep
        const float r = a.rgb[rowo + c], d = a.dep[rowo + c], al = a.alpha[c];
        const bool sr = a.m_rgb[c] != 0.f, sd = a.m_dep[c] != 0.f;
        const float dr = (sr ? 0.f : g0) + (sd ? al * g1v : 0.f);
        a.d_rgb_pre[rowo + c] = r > 0.f ? dr : 0.f;            // input_embed's ReLU (:183)
        a.d_dep[rowo + c] = (sr ? al * g0 : 0.f) + (sd ? 0.f : g1v);
        a.t_dal[rowo + c] = (sr ? g0 * d : 0.f) + (sd ? g1v * r : 0.f);
    }
}

}  // namespace r3d

using namespace r3d;

/* Forward seam of the activation-magnitude fuser: x0 [2N, C] = embd_drop(scaled exchange(rgb, dep)), h1 = norm1(x0),
 * m1 / r1 [2N].  Rows 2n / 2n+1 are frame n's RGB / depth token; drop_mask (optional) indexes x0's elements. */
R3D_EXPORT int r3d_scaled_exchange_fwd(const float* rgb, const float* dep, const float* mask_rgb, const float* mask_dep,
                                       const float* alpha, const uint8_t* drop_mask, float drop_scale,
                                       const float* ln1_gamma, const float* ln1_beta, float* x0, float* h1, float* m1,
                                       float* r1, int N, int C, void* stream) {
    R3D_REQUIRE(rgb && dep && mask_rgb && mask_dep && alpha && ln1_gamma && ln1_beta && x0 && h1 && m1 && r1);
    R3D_REQUIRE(N > 0 && C > 0 && C <= 1024);
    VaryArgs a{};
    a.rgb = rgb; a.dep = dep; a.alpha = alpha; a.m_rgb = mask_rgb; a.m_dep = mask_dep; a.drop = drop_mask;
    a.drop_scale = drop_scale; a.ln1_g = ln1_gamma; a.ln1_b = ln1_beta; a.x0 = x0; a.h1 = h1; a.m1 = m1; a.r1 = r1;
    a.N = N; a.C = C;
    seam_launch(vary_exchange_fwd_kernel<2>, vary_exchange_fwd_kernel<8>, vary_exchange_fwd_kernel<16>, C, dim3(N), dim3(128),
                0, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

/* Backward seam: norm1 backward (+ add1, optional), dropout, adjoint of the scaled exchange.
 *   d_rgb_pre [N, C] = (d_x0_rgb (1 - m_r) + alpha m_d d_x0_dep) [rgb > 0]
 *   d_dep     [N, C] =  d_x0_dep (1 - m_d) + alpha m_r d_x0_rgb
 *   t_dal     [N, C] =  m_r d_x0_rgb dep + m_d d_x0_dep rgb      (column sum = d alpha)
 * ws_n1 (optional) [N][2][C]: norm1 parameter partials per frame (finalize job with rows = -N). */
R3D_EXPORT int r3d_scaled_exchange_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1,
                                       const float* ln1_gamma, const float* add1, const uint8_t* drop_mask,
                                       float drop_scale, const float* rgb, const float* dep, const float* mask_rgb,
                                       const float* mask_dep, const float* alpha, float* d_rgb_pre, float* d_dep,
                                       float* t_dal, float* ws_n1, int N, int C, void* stream) {
    R3D_REQUIRE(d_h1 && x0 && m1 && r1 && ln1_gamma && rgb && dep && mask_rgb && mask_dep && alpha);
    R3D_REQUIRE(d_rgb_pre && d_dep && t_dal && N > 0 && C > 0 && C <= 1024);
    VaryArgs a{};
    a.rgb = rgb; a.dep = dep; a.alpha = alpha; a.m_rgb = mask_rgb; a.m_dep = mask_dep; a.drop = drop_mask;
    a.drop_scale = drop_scale; a.ln1_g = ln1_gamma; a.x0 = const_cast<float*>(x0); a.m1 = const_cast<float*>(m1);
    a.r1 = const_cast<float*>(r1); a.d_h1 = d_h1; a.add1 = add1; a.d_rgb_pre = d_rgb_pre; a.d_dep = d_dep; a.t_dal = t_dal;
    a.ws_n1 = ws_n1; a.N = N; a.C = C;
    seam_launch(vary_exchange_bwd_kernel<2>, vary_exchange_bwd_kernel<8>, vary_exchange_bwd_kernel<16>, C, dim3(N), dim3(128),
                (size_t)6 * C * sizeof(float), (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
