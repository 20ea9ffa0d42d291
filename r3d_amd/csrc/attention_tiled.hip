// Tiled ("flash"-style) fp32 attention core for the query models' S x S decoder attentions (engine_unsup.py): any
// Lq, Lk >= 1 and any head width 1 <= dh <= 128, same operand conventions as r3d_mha_core_* (attention.hip), but no
// [Lq][Lk] tensor is ever written to memory: the forward streams 64-key tiles through LDS under an online softmax and
// keeps only o and lse = m + log l per query row; the backward recomputes P = exp(s - lse) tile by tile.
//
// All kernels: 256 threads = 4 waves, 64 x 64 score tiles, head width zero-padded in LDS to DP in {16, 32, 64, 128}.
// Wave w owns rows [16w, 16w + 16) of the tile: its 16 x 64 scores, its row statistics and its 16 x DP accumulators, so
// every product is a chain of fp32-input 16x16x4 MFMAs on LDS operands (exact fp32, one VGPR per operand).  Each lane
// feeds FOUR k-steps from one 16-byte LDS read: step t of lane (c, kq) carries k = k0 + 4 kq + t on both operands, a
// permutation of the k order inside a 16-wide group that A and B share.
//
//   forward   grid (ceil(Lq / 64), heads, B): Q resident, K / V tiles streamed; S = Q K^T -> LDS; per row (4 lanes each)
//             m, l update and P' = P o keep * drop_scale -> LDS; O = O * alpha + P' V.
//   backward  two kernels, no atomics, no hand-off between workgroups (results are bitwise reproducible):
//     dq      grid over QUERY tiles: delta = rowsum(dO o O) (written to the workspace), then sweeps the key tiles:
//             dS = P o (dO V^T o keep * drop_scale - delta) * scale -> LDS, dQ += dS K.
//     dkv     grid over KEY tiles (launched after dq: it reads delta): K / V resident, sweeps the query tiles with the
//             TRANSPOSED products (K Q^T, V dO^T, so the key is the accumulator row): dV += P'^T dO, dK += dS^T Q.
// The argument block, the key mask and the host check are attention_lse.h's, shared with the split-key core.
#include "attention_lse.h"

namespace r3d {

// accumulator tiles of wave w -> rows [row0 + 16w, ...) x [0, dh) of a strided matrix (rows past L are not written)
template <int DP>
__device__ __forceinline__ void store_acc(const f32x4 (&acc)[DP / 16], float* base, int ld, int row0, int L, int dh, int w,
                                          int c, int kq) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = row0 + 16 * w + 4 * kq + r;
        if (i >= L) continue;
#pragma unroll
        for (int n = 0; n < DP / 16; ++n)
            if (16 * n + c < dh) base[(size_t)i * ld + 16 * n + c] = acc[n][r];
    }
}

template <int DP>
__global__ __launch_bounds__(256) void mha_tiled_fwd_kernel(const LseArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [64][LD]
    float* Ks = Qs + TT * LD;           // [64][LD]
    float* Vs = Ks + TT * LD;           // [64][LD]
    float* Ss = Vs + TT * LD;           // [64][SLD]  scores, then the dropped probabilities
    float* rowa = Ss + TT * SLD;        // [64]       per-row rescale factor, at the end the row sum
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * TT, h = blockIdx.y, b = blockIdx.z;
    const int Lq = a.Lq, Lk = a.Lk, dh = a.dh;
    const float* qb = a.q + (size_t)b * Lq * a.ldq + h * dh;
    const float* kb = a.k + (size_t)b * Lk * a.ldk + h * dh;
    const float* vb = a.v + (size_t)b * Lk * a.ldv + h * dh;
    const size_t bh = (size_t)b * a.heads + h;
    stage_tile<DP>(Qs, qb, a.ldq, q0, Lq, dh, tid);
    // softmax role: row srow of the tile, columns 4t + part
    const int srow = 16 * w + (lane >> 2), part = lane & 3, si = q0 + srow;
    const size_t drow = (bh * Lq + (size_t)(si < Lq ? si : 0)) * Lk;
    float m = -INFINITY, l = 0.f;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Lk; k0 += TT) {
        __syncthreads();                                        // the previous tile's products are done with Ks / Vs / Ss
        stage_tile<DP>(Ks, kb, a.ldk, k0, Lk, dh, tid);
        stage_tile<DP>(Vs, vb, a.ldv, k0, Lk, dh, tid);
        // the tile's key masks and keep bytes are fetched here, with K / V: one memory round trip per tile, not three
        bool masked[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) masked[t] = key_masked(a, b, k0 + 16 * t + c);
        uint8_t keep[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int j = k0 + 4 * t + part;
            keep[t] = (a.drop && si < Lq && j < Lk) ? a.drop[drow + j] : (uint8_t)1;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(s, Qs + 16 * w * LD, Ks + 16 * t * LD, c, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(16 * w + 4 * kq + r) * SLD + 16 * t + c] = masked[t] ? -INFINITY : s[r] * a.scale;
        }
        __syncthreads();
        {
            float sv[16], mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                sv[t] = Ss[srow * SLD + 4 * t + part];
                mx = fmaxf(mx, sv[t]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1));
            mx = fmaxf(mx, __shfl_xor(mx, 2));
            const float m_new = fmaxf(m, mx);
            // a fully masked tile before any valid key: m_new = -inf; subtracting 0 keeps exp(-inf) = 0 instead of NaN
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            const float alpha = expf(m - m_use);
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                float p = expf(sv[t] - m_use);
                sum += p;
                if (a.drop) p *= a.drop_scale * (float)keep[t];
                Ss[srow * SLD + 4 * t + part] = p;
            }
            l = l * alpha + quad_sum(sum);
            m = m_new;
            if (part == 0) rowa[srow] = alpha;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float al = rowa[16 * w + 4 * kq + r];
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n][r] *= al;
        }
        mma_nn<DP>(acc, Ss + 16 * w * SLD, Vs, c, kq);
    }
    __syncthreads();
    if (part == 0) {
        rowa[srow] = l;
        if (si < Lq) a.lse[bh * Lq + si] = m + logf(l);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lr = rowa[16 * w + 4 * kq + r];              // all keys masked: 0 / 0 = NaN, as in PyTorch
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n][r] = acc[n][r] / lr;
    }
    store_acc<DP>(acc, a.o + (size_t)b * Lq * a.ldo + h * dh, a.ldo, q0, Lq, dh, w, c, kq);
}

template <int DP>
__global__ __launch_bounds__(256) void mha_tiled_bwd_dq_kernel(const LseArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [64][LD]
    float* dOs = Qs + TT * LD;          // [64][LD]
    float* Ks = dOs + TT * LD;          // [64][LD]
    float* Vs = Ks + TT * LD;           // [64][LD]
    float* Ss = Vs + TT * LD;           // [64][SLD]  dS
    float* rowl = Ss + TT * SLD;        // [64] lse of the tile's rows
    float* rowd = rowl + TT;            // [64] delta of the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * TT, h = blockIdx.y, b = blockIdx.z;
    const int Lq = a.Lq, Lk = a.Lk, dh = a.dh;
    const float* qb = a.q + (size_t)b * Lq * a.ldq + h * dh;
    const float* kb = a.k + (size_t)b * Lk * a.ldk + h * dh;
    const float* vb = a.v + (size_t)b * Lk * a.ldv + h * dh;
    const float* dob = a.d_o + (size_t)b * Lq * a.lddo + h * dh;
    const float* ob = a.o + (size_t)b * Lq * a.ldo + h * dh;
    const size_t bh = (size_t)b * a.heads + h;
    stage_tile<DP>(Qs, qb, a.ldq, q0, Lq, dh, tid);
    stage_tile<DP>(dOs, dob, a.lddo, q0, Lq, dh, tid);
    __syncthreads();
    {   // delta = rowsum(dO o O): 4 lanes per row
        const int srow = 16 * w + (lane >> 2), part = lane & 3, si = q0 + srow;
        float s = 0.f;
        if (si < Lq)
            for (int d = part; d < dh; d += 4) s += dOs[srow * LD + d] * ob[(size_t)si * a.ldo + d];
        s = quad_sum(s);
        if (part == 0) {
            rowd[srow] = s;
            rowl[srow] = si < Lq ? a.lse[bh * Lq + si] : 0.f;
            if (si < Lq) a.delta[bh * Lq + si] = s;
        }
    }
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Lk; k0 += TT) {
        __syncthreads();
        stage_tile<DP>(Ks, kb, a.ldk, k0, Lk, dh, tid);
        stage_tile<DP>(Vs, vb, a.ldv, k0, Lk, dh, tid);
        bool live[4][4];                                        // [t][r]; fetched with K / V, as the keep bytes
        uint8_t keep[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = k0 + 16 * t + c;
            const bool masked = key_masked(a, b, j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = q0 + 16 * w + 4 * kq + r;
                live[t][r] = !masked && i < Lq;
                keep[t][r] = (a.drop && live[t][r]) ? a.drop[(bh * Lq + i) * Lk + j] : (uint8_t)1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(s, Qs + 16 * w * LD, Ks + 16 * t * LD, c, kq);
            mma_nt<DP>(dp, dOs + 16 * w * LD, Vs + 16 * t * LD, c, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                const float p = live[t][r] ? expf(s[r] * a.scale - rowl[row]) : 0.f;
                float g = dp[r];
                if (a.drop && live[t][r]) g *= a.drop_scale * (float)keep[t][r];
                Ss[row * SLD + 16 * t + c] = p * (g - rowd[row]) * a.scale;
            }
        }
        __syncthreads();
        mma_nn<DP>(acc, Ss + 16 * w * SLD, Ks, c, kq);
    }
    store_acc<DP>(acc, a.dq + (size_t)b * Lq * a.lddq + h * dh, a.lddq, q0, Lq, dh, w, c, kq);
}

template <int DP>
__global__ __launch_bounds__(256) void mha_tiled_bwd_dkv_kernel(const LseArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ks = lds;                    // [64][LD]
    float* Vs = Ks + TT * LD;           // [64][LD]
    float* Qs = Vs + TT * LD;           // [64][LD]
    float* dOs = Qs + TT * LD;          // [64][LD]
    float* Ss = dOs + TT * LD;          // [64 keys][SLD]  P'^T, then dS^T
    float* rowl = Ss + TT * SLD;        // [64] lse of the query tile's rows
    float* rowd = rowl + TT;            // [64] delta of the query tile's rows
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int k0 = blockIdx.x * TT, h = blockIdx.y, b = blockIdx.z;
    const int Lq = a.Lq, Lk = a.Lk, dh = a.dh;
    const float* qb = a.q + (size_t)b * Lq * a.ldq + h * dh;
    const float* kb = a.k + (size_t)b * Lk * a.ldk + h * dh;
    const float* vb = a.v + (size_t)b * Lk * a.ldv + h * dh;
    const float* dob = a.d_o + (size_t)b * Lq * a.lddo + h * dh;
    const size_t bh = (size_t)b * a.heads + h;
    stage_tile<DP>(Ks, kb, a.ldk, k0, Lk, dh, tid);
    stage_tile<DP>(Vs, vb, a.ldv, k0, Lk, dh, tid);
    bool masked[4];                                              // this lane's 4 accumulator rows are keys
#pragma unroll
    for (int r = 0; r < 4; ++r) masked[r] = key_masked(a, b, k0 + 16 * w + 4 * kq + r);
    f32x4 gk[NT], gv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) gk[n] = gv[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < Lq; q0 += TT) {
        __syncthreads();
        stage_tile<DP>(Qs, qb, a.ldq, q0, Lq, dh, tid);
        stage_tile<DP>(dOs, dob, a.lddo, q0, Lq, dh, tid);
        if (tid < TT) {
            const int i = q0 + tid;
            rowl[tid] = i < Lq ? a.lse[bh * Lq + i] : 0.f;
            rowd[tid] = i < Lq ? a.delta[bh * Lq + i] : 0.f;
        }
        bool live[4][4];                                        // [t][r]; fetched with Q / dO, as the keep bytes
        uint8_t keepb[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = q0 + 16 * t + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                live[t][r] = !masked[r] && i < Lq;
                keepb[t][r] = (a.drop && live[t][r]) ? a.drop[(bh * Lq + i) * Lk + k0 + 16 * w + 4 * kq + r] : (uint8_t)1;
            }
        }
        __syncthreads();
        f32x4 pT[4], dsT[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(s, Ks + 16 * w * LD, Qs + 16 * t * LD, c, kq);        // [key][query]
            mma_nt<DP>(dp, Vs + 16 * w * LD, dOs + 16 * t * LD, c, kq);
            const float li = rowl[16 * t + c], di = rowd[16 * t + c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = live[t][r] ? expf(s[r] * a.scale - li) : 0.f;
                float keep = 1.f;
                if (a.drop && live[t][r]) keep = a.drop_scale * (float)keepb[t][r];
                pT[t][r] = p * keep;
                dsT[t][r] = p * (dp[r] * keep - di) * a.scale;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(16 * w + 4 * kq + r) * SLD + 16 * t + c] = pT[t][r];
        __syncthreads();
        mma_nn<DP>(gv, Ss + 16 * w * SLD, dOs, c, kq);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(16 * w + 4 * kq + r) * SLD + 16 * t + c] = dsT[t][r];
        __syncthreads();
        mma_nn<DP>(gk, Ss + 16 * w * SLD, Qs, c, kq);
    }
    store_acc<DP>(gk, a.dk + (size_t)b * Lk * a.lddk + h * dh, a.lddk, k0, Lk, dh, w, c, kq);
    store_acc<DP>(gv, a.dv + (size_t)b * Lk * a.lddv + h * dh, a.lddv, k0, Lk, dh, w, c, kq);
}

// The shapes the tiled pair runs: the single statement of its limits (r3d_mha_tiled_supported, and both launches).
static bool tiled_shape_ok(int Lq, int Lk, int dh, bool /*bwd*/) { return Lq >= 1 && Lk >= 1 && dh >= 1 && dh <= 128; }

static size_t tiled_lds_bytes(int dp, bool bwd) {
    return ((size_t)(bwd ? 4 : 3) * TT * (dp + 4) + (size_t)TT * SLD + (bwd ? 2 : 1) * TT) * sizeof(float);
}

template <int DP>
static int tiled_launch(const LseArgs& a, bool bwd, hipStream_t s) {
    const size_t lds = tiled_lds_bytes(DP, bwd);
    const dim3 gq(r3d_cdiv(a.Lq, TT), a.heads, a.B), gk(r3d_cdiv(a.Lk, TT), a.heads, a.B), blk(256);
    if (!bwd) {
        hipError_t e = allow_dynamic_lds((const void*)mha_tiled_fwd_kernel<DP>, lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(mha_tiled_fwd_kernel<DP>, gq, blk, lds, s, a);
        R3D_LAUNCH_CHECK();
        return R3D_OK;
    }
    hipError_t e = allow_dynamic_lds((const void*)mha_tiled_bwd_dq_kernel<DP>, lds);
    if (e == hipSuccess) e = allow_dynamic_lds((const void*)mha_tiled_bwd_dkv_kernel<DP>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mha_tiled_bwd_dq_kernel<DP>, gq, blk, lds, s, a);       // writes delta ...
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(mha_tiled_bwd_dkv_kernel<DP>, gk, blk, lds, s, a);      // ... which this one reads
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

static int tiled_dispatch(LseArgs a, bool bwd, void* stream) {
    int rc = lse_admit(a, tiled_shape_ok(a.Lq, a.Lk, a.dh, bwd), bwd, false);
    if (rc != R3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (tile_dp(a.dh)) {
        case 16: return tiled_launch<16>(a, bwd, s);
        case 32: return tiled_launch<32>(a, bwd, s);
        case 64: return tiled_launch<64>(a, bwd, s);
        default: return tiled_launch<128>(a, bwd, s);
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_mha_tiled_supported(int Lq, int Lk, int dh, int bwd) { return tiled_shape_ok(Lq, Lk, dh, bwd != 0) ? 1 : 0; }

R3D_EXPORT int r3d_mha_tiled_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                 const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx,
                                 const uint8_t* drop_mask, float drop_scale, float* o, int ldo, float* lse, int B, int heads,
                                 int Lq, int Lk, int dh, void* stream) {
    return tiled_dispatch(lse_args(q, ldq, k, ldk, v, ldv, key_padding_mask, key_label, pad_idx, drop_mask, drop_scale, o, ldo, lse,
                                   nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, B, heads, Lq, Lk, dh),
                          false, stream);
}

R3D_EXPORT int r3d_mha_tiled_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                 const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx,
                                 const uint8_t* drop_mask, float drop_scale, const float* o, int ldo, const float* lse,
                                 const float* d_o, int lddo, float* delta, float* dq, int lddq, float* dk, int lddk, float* dv,
                                 int lddv, int B, int heads, int Lq, int Lk, int dh, void* stream) {
    return tiled_dispatch(lse_args(q, ldq, k, ldk, v, ldv, key_padding_mask, key_label, pad_idx, drop_mask, drop_scale, o, ldo, lse,
                                   d_o, lddo, delta, dq, lddq, dk, lddk, dv, lddv, nullptr, B, heads, Lq, Lk, dh),
                          true, stream);
}
