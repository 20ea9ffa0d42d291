// The seam between the THREE input embeddings (RGB, depth, gaze) and the three-modality SA-Fuser block, one launch per
// direction -- the fifth seam family on seam_rows.h (build-defined, like fuser3.hip: the reference's CMFuser is two-token).
//   forward : split-K slab sums of the RGB and depth projections (+bias; ReLU on RGB, LayerNorm + ReLU on depth, the
//             conventions of r3d_embed_fuse_fwd), the gaze embedding relu(LN_g(b_g + W_g . gaze[n])) (the depth branch's
//             form, futr_safuser_tokenfusion.py:194-197, on a [gaze_dim] input), the cyclic exchange (modality m takes the
//             masked columns of modality (m + 1) mod 3) + embd_drop, fuser.blocks.0.norm1.
//   backward: norm1's adjoint (+ the two residual gradients), dropout, the exchange adjoint (a column taken from the next
//             modality sends its gradient there), the three ReLU gates and both LayerNorm adjoints.
// Rows are frame-major as in fuser3.hip: tokens of frame n are rows 3n (rgb), 3n + 1 (depth), 3n + 2 (gaze).
//
// THREE WAVES OWN A FRAME, one modality each, and pass the exchanged columns through LDS.  The other choice -- one wave
// rebuilding all three embeddings, as the two tail waves of embed_seam.h rebuild both -- keeps three rows live beside the
// operands of two LayerNorms and norm1: 3 x 16 values more per lane at EPL 16, and the third LayerNorm's two wave
// reductions on every wave's chain.  Here a wave holds its own row only; the price is one LDS row per modality and one
// more barrier.  (Register figures of both kernels: DESIGN.md section 4.)
// The forward's workgroups stride over the frames, so W_g is staged ONCE per workgroup, transposed ([G][H]: lane l reads
// column l + 64 e of input j, consecutive words) -- 32 KiB at hidden 1024, gaze_dim 8.
// No atomics; every sum has a fixed order (wave shuffles, fixed-order LDS sums): the same call gives the same bits.
#include "common.h"
#include "../../include/r3d_hip.h"
#include "seam_rows.h"

namespace r3d {

constexpr int kFuse3MaxGaze = 8;
constexpr int kFuse3MaxGrid = 1024;        // forward workgroups; frames past it are taken in a stride loop

struct Fuse3FwdArgs {
    const float* rgb_src; int ns_r; const float* bias_r;      // ns_r > 0: [ns_r][N][H] slabs, bias + ReLU applied here
    const float* dep_src; int ns_d; const float* bias_d;      // [ns_d][N][H] slabs (+bias); LN + ReLU here
    const float* lnd_g; const float* lnd_b;
    const float* gaze; const float* w_g; const float* b_g; const float* lng_g; const float* lng_b; int G;
    const float* mask;                                         // [3][H] 1.0 / 0.0
    const uint8_t* drop; float drop_scale; const float* ln1_g; const float* ln1_b;
    float* rgb_out; float* dep_pre; float* mean_d; float* rstd_d; float* dep_out;
    float* gz_pre; float* mean_g; float* rstd_g; float* gz_out;
    float* x0; float* h1; float* m1; float* r1;
    int N, H;
};

// LDS: WgT [G][H] | red [4 waves][2 projections][H] | E [3][H]
template <int EPL>
__global__ __launch_bounds__(256) void embed_fuse3_fwd_kernel(const Fuse3FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H = a.H, G = a.G;
    float* WgT = lds;
    float* red = lds + (size_t)G * H;
    float* E = red + (size_t)8 * H;
    for (int i = threadIdx.x; i < H * G; i += 256) WgT[(i % G) * H + i / G] = a.w_g[i];
    const size_t stride = (size_t)a.N * H;
    int cc[EPL];
    seam_cols<EPL>(lane, H, cc);
    const int m = wave < 3 ? wave : 0;          // (wave 3 only sums slabs; its row operands are loaded and unused)
    for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
        const size_t rowo = (size_t)n * H, row = (size_t)3 * n + m;
        // ---- loads of the row tail, issued before the slab sums
        float keep[EPL], gzin[kFuse3MaxGaze];
#pragma unroll
        for (int e = 0; e < EPL; ++e) keep[e] = a.drop ? a.drop_scale * (float)a.drop[row * H + cc[e]] : 1.f;
#pragma unroll
        for (int j = 0; j < kFuse3MaxGaze; ++j) gzin[j] = a.gaze[(size_t)n * G + (j < G ? j : G - 1)];
        // ---- slab sums: wave w takes slabs w, w + 4, ... of both projections in order; a slab's EPL columns are in flight
        // together
        float ar[EPL], ad[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) { ar[e] = 0.f; ad[e] = 0.f; }
        if (a.ns_r > 0) {
            for (int s = wave; s < a.ns_r; s += 4) {
                const float* p = a.rgb_src + (size_t)s * stride + rowo;
#pragma unroll
                for (int e = 0; e < EPL; ++e) ar[e] += p[cc[e]];
            }
        } else if (wave == 0) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) ar[e] = a.rgb_src[rowo + cc[e]];
        }
        for (int s = wave; s < a.ns_d; s += 4) {
            const float* p = a.dep_src + (size_t)s * stride + rowo;
#pragma unroll
            for (int e = 0; e < EPL; ++e) ad[e] += p[cc[e]];
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if (c < H) {
                red[((size_t)wave * 2 + 0) * H + c] = ar[e];
                red[((size_t)wave * 2 + 1) * H + c] = ad[e];
            }
        }
        // ---- the row tail's vector operands, in flight across the barrier (loaded per frame: held over the slab sums
        // they cost the widest instance 96 registers)
        float g1[EPL], b1[EPL], lg[EPL], lb[EPL], bs[EPL], msk[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            g1[e] = a.ln1_g[cc[e]]; b1[e] = a.ln1_b[cc[e]];
            lg[e] = (m == 2 ? a.lng_g : a.lnd_g)[cc[e]];
            lb[e] = (m == 2 ? a.lng_b : a.lnd_b)[cc[e]];
            const float* bp = m == 0 ? (a.ns_r > 0 ? a.bias_r : nullptr) : (m == 1 ? a.bias_d : a.b_g);
            bs[e] = bp ? bp[cc[e]] : 0.f;
            msk[e] = a.mask[(size_t)m * H + cc[e]];
        }
        __syncthreads();
        // ---- wave m finishes embedding m: RGB bias + ReLU; depth / gaze LayerNorm + ReLU
        float v[EPL];
        if (wave < 3) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int c = lane + 64 * e;
                float t = 0.f;
                if (c < H) {
                    if (m == 2) {
                        t = bs[e];
#pragma unroll
                        for (int j = 0; j < kFuse3MaxGaze; ++j)
                            if (j < G) t += WgT[j * H + c] * gzin[j];
                    } else {
                        t = (red[(0 + m) * H + c] + red[(2 + m) * H + c]) + (red[(4 + m) * H + c] + red[(6 + m) * H + c]);
                        if (m == 1 || a.ns_r > 0) t += bs[e];
                    }
                }
                v[e] = t;
            }
            if (m == 0) {
                if (a.ns_r > 0) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) v[e] = fmaxf(v[e], 0.f);
                }
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int c = lane + 64 * e;
                    if (c < H) {
                        if (a.rgb_out != a.rgb_src) a.rgb_out[rowo + c] = v[e];
                        E[c] = v[e];
                    }
                }
            } else {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < EPL; ++e) s += v[e];
                const float mean = wave_sum(s) / (float)H;
                float q = 0.f;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const float dl = lane + 64 * e < H ? v[e] - mean : 0.f;
                    q += dl * dl;
                }
                const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + kSeamLnEps);
                float* pre = m == 1 ? a.dep_pre : a.gz_pre;
                float* out = m == 1 ? a.dep_out : a.gz_out;
                if (lane == 0) { (m == 1 ? a.mean_d : a.mean_g)[n] = mean; (m == 1 ? a.rstd_d : a.rstd_g)[n] = rstd; }
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int c = lane + 64 * e;
                    const float y = fmaxf((v[e] - mean) * rstd * lg[e] + lb[e], 0.f);
                    if (c < H) { pre[rowo + c] = v[e]; out[rowo + c] = y; E[(size_t)m * H + c] = y; }
                    v[e] = y;
                }
            }
        }
        __syncthreads();
        // ---- token m of the frame: the masked columns come from modality (m + 1) mod 3; embd_drop; norm1
        if (wave < 3) {
            const float* nxt = E + (size_t)(m == 2 ? 0 : m + 1) * H;
            float x[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int c = lane + 64 * e;
                float t = 0.f;
                if (c < H) {
                    t = (msk[e] != 0.f ? nxt[c] : v[e]) * keep[e];
                    a.x0[row * H + c] = t;
                }
                x[e] = t;
            }
            seam_norm1_fwd<EPL>(x, g1, b1, a.m1, a.r1, a.h1, row, lane, H);
        }
        // (the next frame writes `red` before its first barrier and E after it; E's readers above are past both of this
        //  frame's barriers and `red` has none left)
    }
}

struct Fuse3BwdArgs {
    const float* d_h1; const float* x0; const float* m1; const float* r1; const float* ln1_g;
    const float* add1; const float* add2; const uint8_t* drop; float drop_scale;
    const float* mask; const float* rgb;
    const float* dep_pre; const float* mean_d; const float* rstd_d; const float* lnd_g; const float* lnd_b;
    const float* gz_pre; const float* mean_g; const float* rstd_g; const float* lng_g; const float* lng_b;
    float* d_rgb_pre; float* d_dep_pre; float* d_gz_pre;
    float* ws_n1; float* ws_dep; float* ws_gz;                 // [N][2][H] partial (dgamma, dbeta)
    int N, H;
};

// One workgroup of three waves per frame; wave t runs token row 3n + t through norm1's adjoint, then modality t.
// LDS: G [3][H] | P [3][2][H]
template <int EPL>
__global__ __launch_bounds__(192) void embed_fuse3_bwd_kernel(const Fuse3BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.x, lane = threadIdx.x & 63, t = threadIdx.x >> 6, H = a.H;
    float* G = lds;
    float* P = lds + 3 * H;
    const size_t row = (size_t)3 * n + t, rowo = (size_t)n * H;
    const int tp = t == 0 ? 2 : t - 1;         // the modality that took ITS masked columns from this one
    int cc[EPL];
    seam_cols<EPL>(lane, H, cc);
    SeamRowBwd<EPL, true, false> tk;
    tk.load(a.d_h1, a.x0, a.m1, a.r1, a.ln1_g, a.add1, a.add2, a.drop, a.drop_scale, row, H, cc);
    SeamDepthLnBwd<EPL> dl;
    float mo[EPL], mp[EPL], rg[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        mo[e] = a.mask[(size_t)t * H + cc[e]];
        mp[e] = a.mask[(size_t)tp * H + cc[e]];
        rg[e] = t == 0 ? a.rgb[rowo + cc[e]] : 1.f;
    }
    if (t == 1) dl.load(a.dep_pre, a.mean_d, a.rstd_d, a.lnd_g, a.lnd_b, n, H, cc);
    if (t == 2) dl.load(a.gz_pre, a.mean_g, a.rstd_g, a.lng_g, a.lng_b, n, H, cc);
    tk.norm1_bwd(G, P, t, lane, H, cc);
    __syncthreads();
    // ---- exchange adjoint: modality t keeps its own slot where unmasked and is fed by the previous modality's slot
    // where that one is masked (select, not a 0/1 product: a gated-off gradient is +0.0)
    float dd[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        dd[e] = 0.f;
        if (c < H) dd[e] = (mo[e] != 0.f ? 0.f : G[t * H + c]) + (mp[e] != 0.f ? G[tp * H + c] : 0.f);
    }
    if (t == 0) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if (c < H) {
                a.d_rgb_pre[rowo + c] = rg[e] > 0.f ? dd[e] : 0.f;
                // norm1's parameter-gradient partial of the frame: its three token rows in order
                a.ws_n1[((size_t)n * 2 + 0) * H + c] = (P[0 * H + c] + P[2 * H + c]) + P[4 * H + c];
                a.ws_n1[((size_t)n * 2 + 1) * H + c] = (P[1 * H + c] + P[3 * H + c]) + P[5 * H + c];
            }
        }
    } else if (t == 1) {
        dl.ln_relu_bwd(dd, a.d_dep_pre, a.ws_dep, n, lane, H);
    } else {
        dl.ln_relu_bwd(dd, a.d_gz_pre, a.ws_gz, n, lane, H);
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_embed_fuse3_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                                   const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* gaze,
                                   const float* w_gaze, const float* b_gaze, const float* lng_gamma, const float* lng_beta,
                                   int gaze_dim, const float* mask, const uint8_t* drop_mask, float drop_scale,
                                   const float* ln1_gamma, const float* ln1_beta, float* rgb_out, float* dep_pre_out,
                                   float* mean_d, float* rstd_d, float* dep_out, float* gz_pre_out, float* mean_g,
                                   float* rstd_g, float* gz_out, float* x0, float* h1, float* m1, float* r1, int N, int H,
                                   void* stream) {
    R3D_REQUIRE(rgb_src && dep_src && lnd_gamma && lnd_beta && gaze && w_gaze && b_gaze && lng_gamma && lng_beta && mask);
    R3D_REQUIRE(ln1_gamma && ln1_beta && rgb_out && dep_pre_out && mean_d && rstd_d && dep_out && gz_pre_out && mean_g && rstd_g);
    R3D_REQUIRE(gz_out && x0 && h1 && m1 && r1);
    R3D_REQUIRE(N > 0 && H > 0 && H <= 1024 && ns_r >= 0 && ns_d >= 1 && gaze_dim >= 1 && gaze_dim <= kFuse3MaxGaze);
    R3D_REQUIRE(ns_r == 0 || bias_r);
    Fuse3FwdArgs a{rgb_src, ns_r, bias_r, dep_src, ns_d, bias_d, lnd_gamma, lnd_beta, gaze, w_gaze, b_gaze, lng_gamma,
                   lng_beta, gaze_dim, mask, drop_mask, drop_scale, ln1_gamma, ln1_beta, rgb_out, dep_pre_out, mean_d, rstd_d,
                   dep_out, gz_pre_out, mean_g, rstd_g, gz_out, x0, h1, m1, r1, N, H};
    const size_t lds = (size_t)(gaze_dim + 8 + 3) * H * sizeof(float);       // 76 KiB at hidden 1024, gaze_dim 8
    if (lds > 64 * 1024) {                            // (only the widest instance gets there; per device, so at every call)
        hipError_t e = hipFuncSetAttribute((const void*)embed_fuse3_fwd_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    seam_launch(embed_fuse3_fwd_kernel<2>, embed_fuse3_fwd_kernel<8>, embed_fuse3_fwd_kernel<16>, H,
                dim3(N < kFuse3MaxGrid ? N : kFuse3MaxGrid), dim3(256), lds, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_embed_fuse3_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                                   const float* add1, const float* add2, const uint8_t* drop_mask, float drop_scale,
                                   const float* mask, const float* rgb, const float* dep_pre, const float* mean_d,
                                   const float* rstd_d, const float* lnd_gamma, const float* lnd_beta, const float* gz_pre,
                                   const float* mean_g, const float* rstd_g, const float* lng_gamma, const float* lng_beta,
                                   float* d_rgb_pre, float* d_dep_pre, float* d_gz_pre, float* ws_n1, float* ws_dep,
                                   float* ws_gz, int N, int H, void* stream) {
    R3D_REQUIRE(d_h1 && x0 && m1 && r1 && ln1_gamma && mask && rgb && dep_pre && mean_d && rstd_d && lnd_gamma && lnd_beta);
    R3D_REQUIRE(gz_pre && mean_g && rstd_g && lng_gamma && lng_beta && d_rgb_pre && d_dep_pre && d_gz_pre);
    R3D_REQUIRE(ws_n1 && ws_dep && ws_gz && N > 0 && H > 0 && H <= 1024);
    Fuse3BwdArgs a{d_h1, x0, m1, r1, ln1_gamma, add1, add2, drop_mask, drop_scale, mask, rgb, dep_pre, mean_d, rstd_d,
                   lnd_gamma, lnd_beta, gz_pre, mean_g, rstd_g, lng_gamma, lng_beta, d_rgb_pre, d_dep_pre, d_gz_pre, ws_n1,
                   ws_dep, ws_gz, N, H};
    seam_launch(embed_fuse3_bwd_kernel<2>, embed_fuse3_bwd_kernel<8>, embed_fuse3_bwd_kernel<16>, H, dim3(N), dim3(192),
                (size_t)9 * H * sizeof(float), (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
