// The row pieces that the four fuser seams share (embed.hip + embed_seam.h: token fusion, plainfuse.hip: plain SA-Fuser,
// varyfuse.hip: activation magnitude, bnfuse.hip: BN blend).  Every seam ends its forward in fuser.blocks.0.norm1 and
// begins its backward with norm1's adjoint; what differs is how the two embeddings become the token rows, and that
// stays in each file.  One wave owns one row: lane l holds columns l + 64 e, e < EPL.
// The off-grid-width rule lives here once: a slot past the row is loaded from column H - 1 (so that no load sits under a
// branch) and every sum takes only the columns c < H, column by column -- a test on the slot would pass every
// multiple-of-64 width and fail the others (tests/test_row_widths_gpu.py).
// Reductions are wave shuffles and fixed-order LDS sums: bitwise reproducible.
#pragma once
#include "common.h"

namespace r3d {

constexpr float kSeamLnEps = 1e-5f;         // nn.LayerNorm's default (depth_layernorm, norm1)

template <int EPL>
__device__ __forceinline__ void seam_cols(int lane, int H, int (&cc)[EPL]) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) { const int c = lane + 64 * e; cc[e] = c < H ? c : H - 1; }
}

// A row lives in one wave's registers: EPL 2 up to 128 columns, 8 up to 512, 16 up to 1024 (the entry points refuse more).
template <typename K, typename A>
static void seam_launch(K k2, K k8, K k16, int H, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const A& a) {
    if (H <= 128) hipLaunchKernelGGL(k2, grid, block, lds_bytes, s, a);
    else if (H <= 512) hipLaunchKernelGGL(k8, grid, block, lds_bytes, s, a);
    else hipLaunchKernelGGL(k16, grid, block, lds_bytes, s, a);
}

// ---- forward tail: token row x (zero at c >= H) -> m1 / r1 [row], h1 [row] = norm1(x)
template <int EPL>
__device__ __forceinline__ void seam_norm1_fwd(const float (&x)[EPL], const float (&g1)[EPL], const float (&b1)[EPL],
                                               float* m1, float* r1, float* h1, size_t row, int lane, int H) {
    float s1 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s1 += x[e];
    const float mean1 = wave_sum(s1) / (float)H;
    float q1 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const float dl = lane + 64 * e < H ? x[e] - mean1 : 0.f;
        q1 += dl * dl;
    }
    const float rstd1 = 1.0f / sqrtf(wave_sum(q1) / (float)H + kSeamLnEps);
    if (lane == 0) { m1[row] = mean1; r1[row] = rstd1; }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        if (c < H) h1[row * H + c] = (x[e] - mean1) * rstd1 * g1[e] + b1[e];
    }
}

// ---- backward of one token row through norm1 and embd_drop, in two steps so that a kernel can issue loads of its own
// between them.  kUpFront (embed.hip, plainfuse.hip): load() issues every operand load of the row, so that all loads of
// the workgroup go out before the first use -- those kernels are latency chains with many operands.  !kUpFront
// (varyfuse.hip, bnfuse.hip): load() takes the row's two statistics only and each slot's operands are loaded where
// norm1_bwd() uses them, as those kernels always did: 26 / 48 / 80 (vary) and 28 / 50 / 82 (BN) VGPRs at EPL 2 / 8 / 16,
// where the up-front form takes 62 at EPL 8 and 110 at EPL 16.
// add1 / add2 (optional) are residual gradients added to norm1's input gradient; drop (optional) is embd_drop's keep mask.
template <int EPL, bool kAdd2, bool kUpFront>
struct SeamRowBwd {
    const float* d_h1; const float* x0; const float* ln1_g; const float* add1; const float* add2; const uint8_t* drop;
    float drop_scale, mean1, rstd1;
    size_t rowo;                            // offset of the token row: row * H
    float dh[EPL], xv[EPL], g1[kUpFront ? EPL : 1], a1[EPL], a2[kAdd2 ? EPL : 1], keep[EPL];

    __device__ __forceinline__ void load_slot(int e, int cc) {
        dh[e] = d_h1[rowo + cc];
        xv[e] = x0[rowo + cc];
        if constexpr (kUpFront) g1[e] = ln1_g[cc];
        a1[e] = add1 ? add1[rowo + cc] : 0.f;
        if constexpr (kAdd2) a2[e] = add2 ? add2[rowo + cc] : 0.f;
        keep[e] = drop ? drop_scale * (float)drop[rowo + cc] : 1.f;
    }

    __device__ __forceinline__ void load(const float* d_h1_, const float* x0_, const float* m1, const float* r1,
                                         const float* ln1_g_, const float* add1_, const float* add2_, const uint8_t* drop_,
                                         float drop_scale_, size_t row, int H, const int (&cc)[EPL]) {
        d_h1 = d_h1_; x0 = x0_; ln1_g = ln1_g_; add1 = add1_; add2 = add2_; drop = drop_; drop_scale = drop_scale_;
        rowo = row * H;
        mean1 = m1[row]; rstd1 = r1[row];
        if constexpr (kUpFront) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) load_slot(e, cc[e]);
        }
    }

    // Token t of the frame: P[t][0/1][c] = the (dgamma, dbeta) terms of norm1, G[t][c] = the gradient of the token row
    // before embd_drop.  Both in LDS; the caller's __syncthreads() follows.
    __device__ __forceinline__ void norm1_bwd(float* G, float* P, int t, int lane, int H, const int (&cc)[EPL]) {
        float xh[EPL], gg[EPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if constexpr (!kUpFront) load_slot(e, cc[e]);
            float xhat = 0.f, g = 0.f;
            if (c < H) {
                xhat = (xv[e] - mean1) * rstd1;
                if constexpr (kUpFront) g = dh[e] * g1[e];
                else g = dh[e] * ln1_g[cc[e]];
                P[(t * 2 + 0) * H + c] = dh[e] * xhat;
                P[(t * 2 + 1) * H + c] = dh[e];
            }
            xh[e] = xhat; gg[e] = g;
            s1 += g; s2 += g * xhat;
        }
        s1 = wave_sum(s1) / (float)H;
        s2 = wave_sum(s2) / (float)H;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if (c >= H) continue;
            float v = rstd1 * (gg[e] - s1 - xh[e] * s2) + a1[e];
            if constexpr (kAdd2) v += a2[e];
            G[t * H + c] = v * keep[e];
        }
    }
};

// ---- norm1 parameter-gradient partial of frame n (its two token rows), by one wave after the __syncthreads():
// ws_n1 [n][0/1][c] = (dgamma, dbeta), summed over the frames by r3d_layernorm_bwd_finalize_batched with rows = -N
template <int EPL>
__device__ __forceinline__ void seam_norm1_partials(const float* P, float* ws_n1, int n, int lane, int H) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lane + 64 * e;
        if (c < H) {
            ws_n1[((size_t)n * 2 + 0) * H + c] = P[0 * H + c] + P[2 * H + c];
            ws_n1[((size_t)n * 2 + 1) * H + c] = P[1 * H + c] + P[3 * H + c];
        }
    }
}

// ---- depth LayerNorm + ReLU backward of frame n (embed.hip, plainfuse.hip), load and compute apart as above.
// dd[e]: the gradient of the depth embedding (after its ReLU) at column lane + 64 e, which each seam forms its own way
// in the loop that also writes d_rgb_pre (handing both over as arrays costs embed.hip's widest instance its occupancy).
template <int EPL>
struct SeamDepthLnBwd {
    float mean_d, rstd_d;
    float dp[EPL], gd[EPL], bd[EPL];

    __device__ __forceinline__ void load(const float* dep_pre, const float* mean, const float* rstd, const float* lnd_g,
                                         const float* lnd_b, int n, int H, const int (&cc)[EPL]) {
        mean_d = mean[n]; rstd_d = rstd[n];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            dp[e] = dep_pre[(size_t)n * H + cc[e]];
            gd[e] = lnd_g[cc[e]]; bd[e] = lnd_b[cc[e]];
        }
    }

    // Writes d_dep_pre [n] (gradient before depth_layernorm) and the (dgamma, dbeta) partial ws_dep [n][0/1][c].
    __device__ __forceinline__ void ln_relu_bwd(const float (&dd)[EPL], float* d_dep_pre, float* ws_dep, int n, int lane,
                                                int H) const {
        float xd[EPL], gq[EPL];
        float u1 = 0.f, u2 = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            float xhat = 0.f, g = 0.f;
            if (c < H) {
                float d = dd[e];
                xhat = (dp[e] - mean_d) * rstd_d;
                if (!(xhat * gd[e] + bd[e] > 0.f)) d = 0.f;
                ws_dep[((size_t)n * 2 + 0) * H + c] = d * xhat;
                ws_dep[((size_t)n * 2 + 1) * H + c] = d;
                g = d * gd[e];
            }
            xd[e] = xhat; gq[e] = g;
            u1 += g; u2 += g * xhat;
        }
        u1 = wave_sum(u1) / (float)H;
        u2 = wave_sum(u2) / (float)H;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int c = lane + 64 * e;
            if (c < H) d_dep_pre[(size_t)n * H + c] = rstd_d * (gq[e] - u1 - xd[e] * u2);
        }
    }
};

}  // namespace r3d
