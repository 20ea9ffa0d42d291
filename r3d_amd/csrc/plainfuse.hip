// The plain SA-Fuser of model/futr_safuser_depth.py, the seam between the two input projections and the fuser block:
//   forward : split-K slab sums of both projections (+bias; ReLU on RGB :141; LayerNorm + ReLU on depth :122-124) ->
//             x0 = embd_drop([rgb; dep] + modality_token) (:40-51) -> fuser.blocks.0.norm1 (transformerblock.py:122).
//             The kernel of r3d_embed_fuse_fwd (embed_seam.h) with the token add in place of the exchange.
//   backward: norm1 backward (+ the residual gradient; there is no x_res, :53,59) -> dropout adjoint -> input_embed's ReLU
//             gate and the depth LayerNorm + ReLU backward, the (dgamma, dbeta) partials of norm1 and the depth LayerNorm
//             per frame (the layout of r3d_embed_fuse_bwd), and t_tok [N, H]: the sum of each frame's two post-dropout
//             row gradients, whose column sum is d modality_token.  That sum is left to a fixed-order reduction (a row-sum
//             job of the grouped weight-gradient launch or of the LayerNorm-finalize launch): no atomics, bitwise the same
//             from run to run.
// One workgroup per frame: 4 waves forward (as embed.hip), 2 waves backward (the two tokens of the frame).  The backward's
// norm1 and depth LayerNorm rows are seam_rows.h's; here are the token partial and the ReLU gate.  Every load of the
// workgroup is issued up front, from clamped columns, none under a data-dependent branch.
#include "common.h"
#include "../../include/r3d_hip.h"
#include "embed_seam.h"

namespace r3d {

struct PlainBwdArgs {
    const float* d_h1; const float* x0; const float* m1; const float* r1; const float* ln1_g; const float* add1;
    const uint8_t* drop; float drop_scale;
    const float* rgb; const float* dep_pre; const float* mean_d; const float* rstd_d; const float* lnd_g; const float* lnd_b;
    float* d_rgb_pre; float* d_dep_pre; float* ws_n1; float* ws_dep;     // all NULL: token partials only (after the chain)
    float* t_tok;
    int N, H;
};

template <int EPL>
__global__ __launch_bounds__(128) void plain_fuse_bwd_kernel(const PlainBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];        // G[2][H] | P[2][2][H]
    const int n = blockIdx.x, lane = threadIdx.x & 63, t = threadIdx.x >> 6, H = a.H;
    const bool full = a.d_rgb_pre != nullptr;
    float* G = lds;
    float* P = lds + 2 * H;
    const size_t row = (size_t)2 * n + t, rowo = (size_t)n * H;
    int cc[EPL];
    seam_cols<EPL>(lane, H, cc);
    // ---- every load of the workgroup up front
    SeamRowBwd<EPL, false, true> tk;
    tk.load(a.d_h1, a.x0, a.m1, a.r1, a.ln1_g, a.add1, nullptr, a.drop, a.drop_scale, row, H, cc);
    SeamDepthLnBwd<EPL> dl;
    float rg[EPL];
    if (t == 0 && full) {
        dl.load(a.dep_pre, a.mean_d, a.rstd_d, a.lnd_g, a.lnd_b, n, H, cc);
#pragma unroll
        for (int e = 0; e < EPL; ++e) rg[e] = a.rgb[rowo + cc[e]];
    }
    // ---- norm1 backward of token t (+ the residual gradient), then back through embd_drop
    tk.norm1_bwd(G, P, t, lane, H, cc);
    __syncthreads();
    if (t == 1) {                       // token partial and norm1 parameter-gradient partial of this frame
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if (c < H) a.t_tok[rowo + c] = G[c] + G[H + c];
        }
        if (full) seam_norm1_partials<EPL>(P, a.ws_n1, n, lane, H);
        return;
    }
    if (!full) return;
    // ---- input_embed's ReLU gate; depth LayerNorm + ReLU backward
    float dd[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        dd[e] = 0.f;
        if (c < H) {
            a.d_rgb_pre[rowo + c] = rg[e] > 0.f ? G[c] : 0.f;
            dd[e] = G[H + c];
        }
    }
    dl.ln_relu_bwd(dd, a.d_dep_pre, a.ws_dep, n, lane, H);
}

}  // namespace r3d

using namespace r3d;

/* Forward seam of the plain fuser: as r3d_embed_fuse_fwd (same sources, slab conventions and outputs), with
 * x0 [2N, H] = embd_drop([rgb; dep] + tok) instead of the exchange.  rgb_src: ns_r > 0 -> [ns_r][N][H] slabs of
 * input_embed (bias_r and ReLU applied here), ns_r == 0 -> the finished embedding.  dep_src: [ns_d][N][H] slabs (ns_d >= 1;
 * ns_d = 1: an already summed pre-LayerNorm matrix, bias_d optional).  tok [H].  jobs_device (optional, with njobs and
 * total_blocks): the chain weights' re-split rides as extra workgroups, as r3d_embed_fuse_fwd_planes.  H <= 1024. */
R3D_EXPORT int r3d_plain_fuse_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                                  const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* tok,
                                  const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma, const float* ln1_beta,
                                  float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d, float* dep_out, float* x0,
                                  float* h1, float* m1, float* r1, int N, int H, const r3d_plane_job* jobs_device, int njobs,
                                  int total_blocks, void* stream) {
    R3D_REQUIRE(!jobs_device || (njobs > 0 && total_blocks > 0));
    EmbedFwdArgs a{rgb_src, ns_r, bias_r, dep_src, ns_d, bias_d, lnd_gamma, lnd_beta, nullptr, nullptr, drop_mask,
                   drop_scale, ln1_gamma, ln1_beta, rgb_out, dep_pre_out, mean_d, rstd_d, dep_out, x0, h1, m1, r1, N, H,
                   jobs_device, jobs_device ? njobs : 0, jobs_device ? total_blocks : 0, tok};
    return embed_fuse_fwd_launch<true>(a, (hipStream_t)stream);
}

/* Backward seam of the plain fuser.  d_h1 [2N, H] = gradient w.r.t. norm1's output, add1 (optional) the residual gradient
 * added to norm1's input gradient.  Outputs: t_tok [N, H] (column sum = d modality_token); d_rgb_pre [N, H] (before
 * input_embed's ReLU), d_dep_pre [N, H] (before depth_layernorm) and the partials ws_n1 / ws_dep [N][2][H] (summed with
 * rows = -N by the LayerNorm finalize) -- those four all given, or all NULL for t_tok alone (the hidden-128 fuser chain
 * already wrote them).  H <= 1024. */
R3D_EXPORT int r3d_plain_fuse_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                                  const float* add1, const uint8_t* drop_mask, float drop_scale, const float* rgb,
                                  const float* dep_pre, const float* mean_d, const float* rstd_d, const float* lnd_gamma,
                                  const float* lnd_beta, float* d_rgb_pre, float* d_dep_pre, float* ws_n1, float* ws_dep,
                                  float* t_tok, int N, int H, void* stream) {
    R3D_REQUIRE(d_h1 && x0 && m1 && r1 && ln1_gamma && t_tok && N > 0 && H > 0 && H <= 1024);
    const bool full = d_rgb_pre != nullptr;
    R3D_REQUIRE(full == (d_dep_pre != nullptr) && full == (ws_n1 != nullptr) && full == (ws_dep != nullptr));
    R3D_REQUIRE(!full || (rgb && dep_pre && mean_d && rstd_d && lnd_gamma && lnd_beta));
    PlainBwdArgs a{d_h1, x0, m1, r1, ln1_gamma, add1, drop_mask, drop_scale, rgb, dep_pre, mean_d, rstd_d, lnd_gamma,
                   lnd_beta, d_rgb_pre, d_dep_pre, ws_n1, ws_dep, t_tok, N, H};
    seam_launch(plain_fuse_bwd_kernel<2>, plain_fuse_bwd_kernel<8>, plain_fuse_bwd_kernel<16>, H, dim3(N), dim3(128),
                (size_t)6 * H * sizeof(float), (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
