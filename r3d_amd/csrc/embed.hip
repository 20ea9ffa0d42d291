// The seam between the two input projections and the SA-Fuser block as ONE launch per direction (train mode, where the
// token selection is data independent -- SURVEY F5a):
//   forward : split-K slab sums of both projections (+bias; ReLU on RGB futr_safuser_tokenfusion.py:183; LayerNorm +
//             ReLU on depth :196-197) -> token exchange + embd_drop (:56-62,83) -> fuser.blocks.0.norm1
//             (transformerblock.py:122).   Replaces 4 dependent launches (reduce, LN, exchange, LN) by one.
//   backward: norm1 backward (+ the two residual gradients) -> exchange backward (index_put / clone, ReLU of :183)
//             -> depth LayerNorm + ReLU backward.   Replaces 3 dependent launches by one.
// The forward kernel is a template in embed_seam.h (plainfuse.hip instantiates its token-add form).  What every fuser seam
// does alike -- column setup, width dispatch, norm1 forward and backward rows, the depth LayerNorm backward -- is in
// seam_rows.h; here are the exchange and its adjoint.
// One workgroup (4 waves) per frame row n.  Everything is latency: all loads are unconditional (clamped columns) and
// issued up front.  Reductions are wave shuffles / fixed-order LDS sums -> bitwise reproducible.
#include "common.h"
#include "../../include/r3d_hip.h"
#include "chain_bf3.h"
#include "embed_seam.h"

namespace r3d {

struct EmbedBwdArgs {
    const float* d_h1; const float* x0; const float* m1; const float* r1; const float* ln1_g;
    const float* add1; const float* add2; const uint8_t* drop; float drop_scale;
    const float* m_rgb; const float* m_dep; const float* rgb; const float* dep_pre; const float* mean_d;
    const float* rstd_d; const float* lnd_g; const float* lnd_b;
    float* d_rgb_pre; float* d_dep_pre; float* ws_n1; float* ws_dep;     // ws_*: [N][2][H] partial (dgamma, dbeta)
    int N, H;
};

template <int EPL>
__global__ __launch_bounds__(128) void embed_fuse_bwd_kernel(const EmbedBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];        // G[2][H] | P[2][2][H]
    const int n = blockIdx.x, lane = threadIdx.x & 63, t = threadIdx.x >> 6, H = a.H;
    float* G = lds;
    float* P = lds + 2 * H;
    const size_t row = (size_t)2 * n + t, rowo = (size_t)n * H;
    int cc[EPL];
    seam_cols<EPL>(lane, H, cc);
    // ---- every load of the workgroup up front
    SeamRowBwd<EPL, true, true> tk;
    tk.load(a.d_h1, a.x0, a.m1, a.r1, a.ln1_g, a.add1, a.add2, a.drop, a.drop_scale, row, H, cc);
    SeamDepthLnBwd<EPL> dl;
    float mr[EPL], md[EPL], rg[EPL];
    if (t == 0) {
        dl.load(a.dep_pre, a.mean_d, a.rstd_d, a.lnd_g, a.lnd_b, n, H, cc);
#pragma unroll
        for (int e = 0; e < EPL; ++e) { mr[e] = a.m_rgb[cc[e]]; md[e] = a.m_dep[cc[e]]; rg[e] = a.rgb[rowo + cc[e]]; }
    }
    // ---- norm1 backward of token t (+ the two residual gradients), then back through embd_drop
    tk.norm1_bwd(G, P, t, lane, H, cc);
    __syncthreads();
    if (t == 1) { seam_norm1_partials<EPL>(P, a.ws_n1, n, lane, H); return; }
    // ---- exchange backward (index_put / clone), ReLU of the RGB embedding, depth LayerNorm + ReLU backward
    // (the gate is a 0/1 product: a gated-off negative gradient is -0.0, where plainfuse.hip's select gives +0.0)
    float dd[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        dd[e] = 0.f;
        if (c < H) {
            const float g0 = G[c], g1v = G[H + c];
            a.d_rgb_pre[rowo + c] = ((mr[e] != 0.f ? 0.f : g0) + (md[e] != 0.f ? g1v : 0.f)) * (rg[e] > 0.f ? 1.f : 0.f);
            dd[e] = (mr[e] != 0.f ? g0 : 0.f) + (md[e] != 0.f ? 0.f : g1v);
        }
    }
    dl.ln_relu_bwd(dd, a.d_dep_pre, a.ws_dep, n, lane, H);
}

}  // namespace r3d

using namespace r3d;

/* Backward seam (see the file header): d_h1 [2N,H] = gradient w.r.t. norm1's output; add1 / add2 (optional) are added
 * to norm1's input gradient (the residual paths).  Outputs: d_rgb_pre [N,H] (gradient before input_embed's ReLU),
 * d_dep_pre [N,H] (gradient before depth_layernorm), and the LayerNorm parameter-gradient partials ws_n1 / ws_dep, each
 * [N][2][H] floats: one (dgamma, dbeta) pair per frame, summed by r3d_layernorm_bwd_finalize_batched with rows = -N. */
R3D_EXPORT int r3d_embed_fuse_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                                  const float* add1, const float* add2, const uint8_t* drop_mask, float drop_scale,
                                  const float* mask_rgb, const float* mask_dep, const float* rgb, const float* dep_pre,
                                  const float* mean_d, const float* rstd_d, const float* lnd_gamma, const float* lnd_beta,
                                  float* d_rgb_pre, float* d_dep_pre, float* ws_n1, float* ws_dep, int N, int H,
                                  void* stream) {
    R3D_REQUIRE(d_h1 && x0 && m1 && r1 && ln1_gamma && mask_rgb && mask_dep && rgb && dep_pre && mean_d && rstd_d);
    R3D_REQUIRE(lnd_gamma && lnd_beta && d_rgb_pre && d_dep_pre && ws_n1 && ws_dep && N > 0 && H > 0 && H <= 1024);
    EmbedBwdArgs a{d_h1, x0, m1, r1, ln1_gamma, add1, add2, drop_mask, drop_scale, mask_rgb, mask_dep, rgb, dep_pre,
                   mean_d, rstd_d, lnd_gamma, lnd_beta, d_rgb_pre, d_dep_pre, ws_n1, ws_dep, N, H};
    seam_launch(embed_fuse_bwd_kernel<2>, embed_fuse_bwd_kernel<8>, embed_fuse_bwd_kernel<16>, H, dim3(N), dim3(128),
                (size_t)6 * H * sizeof(float), (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_embed_fuse_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                                  const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* mask_rgb,
                                  const float* mask_dep, const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma,
                                  const float* ln1_beta, float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d,
                                  float* dep_out, float* x0, float* h1, float* m1, float* r1, int N, int H, void* stream) {
    EmbedFwdArgs a{rgb_src, ns_r, bias_r, dep_src, ns_d, bias_d, lnd_gamma, lnd_beta, mask_rgb, mask_dep, drop_mask,
                   drop_scale, ln1_gamma, ln1_beta, rgb_out, dep_pre_out, mean_d, rstd_d, dep_out, x0, h1, m1, r1, N, H,
                   nullptr, 0, 0, nullptr};
    return embed_fuse_fwd_launch<false>(a, (hipStream_t)stream);
}

/* r3d_embed_fuse_fwd + r3d_weight_planes(jobs_device, njobs, total_blocks) in ONE launch: the re-split of the chain weights
 * (which depends on the parameters only) rides as extra workgroups of the seam, whose own 128 workgroups are latency-bound
 * and leave half the chip idle. */
R3D_EXPORT int r3d_embed_fuse_fwd_planes(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                                         const float* bias_d, const float* lnd_gamma, const float* lnd_beta,
                                         const float* mask_rgb, const float* mask_dep, const uint8_t* drop_mask,
                                         float drop_scale, const float* ln1_gamma, const float* ln1_beta, float* rgb_out,
                                         float* dep_pre_out, float* mean_d, float* rstd_d, float* dep_out, float* x0, float* h1,
                                         float* m1, float* r1, int N, int H, const r3d_plane_job* jobs_device, int njobs,
                                         int total_blocks, void* stream) {
    R3D_REQUIRE(jobs_device && njobs > 0 && total_blocks > 0);
    EmbedFwdArgs a{rgb_src, ns_r, bias_r, dep_src, ns_d, bias_d, lnd_gamma, lnd_beta, mask_rgb, mask_dep, drop_mask,
                   drop_scale, ln1_gamma, ln1_beta, rgb_out, dep_pre_out, mean_d, rstd_d, dep_out, x0, h1, m1, r1, N, H,
                   jobs_device, njobs, total_blocks, nullptr};
    return embed_fuse_fwd_launch<false>(a, (hipStream_t)stream);
}
