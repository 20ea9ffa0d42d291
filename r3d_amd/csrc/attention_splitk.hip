// Split-key fp32 attention core for FEW queries against MANY keys: the token-fusion decoder's cross-attention (n_query
// rows per clip against the S frames of the memory) past the LDS of r3d_mha_core_* (attention.hip).  1 <= Lq <= 16, any
// Lk >= 1, 1 <= dh <= 128; operands, masks, dropout keep-mask, o, lse and delta exactly as r3d_mha_tiled_*
// (attention_tiled.hip), so the two pairs are interchangeable on the same buffers.
//
// The tiled core gives wave w the query rows [16w, 16w + 16): with 8 queries one wave of four works, on B * heads
// workgroups that each walk every key tile.  Here the KEYS are spread over the chip: grid (ceil(Lk / chunk), heads, B),
// chunk = r3d_mha_splitk_chunk(Lk, dh) keys per workgroup, and inside a workgroup the key is the MFMA accumulator ROW
// and the (at most 16, zero-padded) queries are the one 16-wide column block -- the transposed form K Q^T of the tiled
// dkv kernel, on tile_mma.h's staging and fp32-input 16x16x4 MFMAs.  Per 64-key tile wave w owns the keys [16w, 16w + 16)
// whatever Lq is.  Lane (c, kq) of a wave then holds s[r] = score(key 16w + 4kq + r, query c): the four values ARE the
// A operand of the next product with the query as its row, k-step r carrying key 4kq + r on both operands (a permutation
// of the k order that A and B share), so P never crosses LDS on the way to P V, nor dS on the way to dS K.
//
//   forward   each wave runs an online softmax over its own keys (row statistics per query: 4 values + two xor
//             shuffles, no barrier); at the end the four waves' (m, l, acc) are merged in wave order through LDS and the
//             workgroup writes its chunk maximum, chunk sum and the unnormalised sum exp(s - m_c) keep drop_scale v for
//             the Lq rows to ws.  A second launch merges the chunks in chunk order into o and lse.
//   backward  each workgroup recomputes delta = rowsum(dO o O) itself, P = exp(s - lse) for its keys, writes dk and dv of
//             its keys (each element once: P'^T and dS^T go through a wave-private 16 x 16 LDS tile to become A operands
//             with the key as the row) and its dq partial to ws; a second launch sums the partials in chunk order and
//             writes delta.
// No atomics, no workgroup waits on another, every sum has a fixed order: the same call gives the same bits.
// The argument block, the key mask and the host check are attention_lse.h's, shared with the tiled core.
#include "attention_lse.h"

#ifndef R3D_SPLITK_CHUNK
#define R3D_SPLITK_CHUNK 128       // keys per workgroup (a multiple of 64); see DESIGN.md for the values tried
#endif

namespace r3d {

constexpr int SKQ = 16;            // query rows of the one column block
constexpr int PLD = 20;            // row stride of a wave's 16 x 16 transposition tile

// delta of query row q: 4 lanes per row (part = 0..3), the order of the tiled dq kernel
__device__ __forceinline__ float sk_delta(const float* dob, int lddo, const float* ob, int ldo, int q, int Lq, int dh, int part) {
    float s = 0.f;
    if (q < Lq)
        for (int d = part; d < dh; d += 4) s += dob[(size_t)q * lddo + d] * ob[(size_t)q * ldo + d];
    return quad_sum(s);
}

// the four waves' 16 x DP accumulator tiles (rows = queries) -> LDS [4][16][DP]
template <int DP>
__device__ __forceinline__ void park_acc(float* Wa, const f32x4 (&acc)[DP / 16], int w, int c, int kq) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int n = 0; n < DP / 16; ++n) Wa[(w * SKQ + 4 * kq + r) * DP + 16 * n + c] = acc[n][r];
}

template <int DP>
__global__ __launch_bounds__(256) void mha_splitk_fwd_kernel(const LseArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [16][LD]
    float* Ks = Qs + SKQ * LD;          // [64][LD]
    float* Vs = Ks + TT * LD;           // [64][LD]
    float* Wa = Ks;                     // after the sweep, over Ks / Vs: [4][16][DP] the waves' accumulators,
    float* Wm = Wa + 4 * SKQ * DP;      // [4][16] their maxima
    float* Wl = Wm + 4 * SKQ;           // [4][16] and sums
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int ch = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int Lq = a.Lq, Lk = a.Lk, dh = a.dh;
    const float* qb = a.q + (size_t)b * Lq * a.ldq + h * dh;
    const float* kb = a.k + (size_t)b * Lk * a.ldk + h * dh;
    const float* vb = a.v + (size_t)b * Lk * a.ldv + h * dh;
    const size_t bh = (size_t)b * a.heads + h;
    stage_tile<DP, SKQ>(Qs, qb, a.ldq, 0, Lq, dh, tid);
    const int kbeg = ch * a.chunk, kend = min(Lk, kbeg + a.chunk);
    const size_t drow = (bh * Lq + (size_t)(c < Lq ? c : 0)) * Lk;
    float m = -INFINITY, l = 0.f;       // of query c over this wave's keys so far (the same on the 4 lanes kq of a column)
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += TT) {
        __syncthreads();                                        // the previous tile's products are done with Ks / Vs
        stage_tile<DP>(Ks, kb, a.ldk, k0, Lk, dh, tid);
        stage_tile<DP>(Vs, vb, a.ldv, k0, Lk, dh, tid);
        bool masked[4];                                         // this lane's 4 keys; fetched with K / V
        uint8_t keep[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = k0 + 16 * w + 4 * kq + r;
            masked[r] = key_masked(a, b, j);
            keep[r] = (a.drop && c < Lq && j < Lk) ? a.drop[drow + j] : (uint8_t)1;
        }
        __syncthreads();
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        mma_nt<DP>(s, Ks + 16 * w * LD, Qs, c, kq);             // [key][query]
        float sv[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sv[r] = masked[r] ? -INFINITY : s[r] * a.scale;
            mx = fmaxf(mx, sv[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);
        // only masked keys so far: m_new = -inf; subtracting 0 keeps exp(-inf) = 0 instead of NaN
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = expf(m - m_use);
        float p[4], sum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = expf(sv[r] - m_use);
            sum += p[r];
            if (a.drop) p[r] *= a.drop_scale * (float)keep[r];
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        l = l * alpha + sum;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                           // accumulator row 4kq + r is a query: its factor lives on lane c = 4kq + r
            const float al = __shfl(alpha, 4 * kq + r);
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n][r] *= al;
        }
        const float* vp = Vs + (16 * w + 4 * kq) * LD + c;      // O[query][d] += P'[query][key] V[key][d], P' from registers
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], vp[r * LD + 16 * n], acc[n], 0, 0, 0);
    }
    __syncthreads();
    park_acc<DP>(Wa, acc, w, c, kq);
    if (kq == 0) {
        Wm[w * SKQ + c] = m;
        Wl[w * SKQ + c] = l;
    }
    __syncthreads();
    // chunk partial: m_c [Lq], l_c [Lq], acc_c [Lq][dh]; the waves merged in wave order
    float* part = a.ws + (bh * a.nchunk + ch) * (size_t)Lq * (dh + 2);
    for (int e = tid; e < Lq * dh; e += 256) {
        const int q = e / dh, d = e % dh;
        float mc = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) mc = fmaxf(mc, Wm[u * SKQ + q]);
        const float mu = mc == -INFINITY ? 0.f : mc;
        float o = 0.f, lc = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float f = expf(Wm[u * SKQ + q] - mu);
            o += Wa[(u * SKQ + q) * DP + d] * f;
            lc += Wl[u * SKQ + q] * f;
        }
        part[2 * Lq + e] = o;
        if (d == 0) {
            part[q] = mc;
            part[Lq + q] = lc;
        }
    }
}

// o = sum_c acc_c exp(m_c - m) / sum_c l_c exp(m_c - m), lse = m + log l; one thread per output element, chunk order
__global__ __launch_bounds__(256) void mha_splitk_fwd_combine_kernel(const LseArgs a) {
    const int Lq = a.Lq, dh = a.dh, h = blockIdx.y, b = blockIdx.z;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Lq * dh) return;
    const int q = e / dh, d = e % dh;
    const size_t bh = (size_t)b * a.heads + h, P = (size_t)Lq * (dh + 2);
    const float* base = a.ws + bh * a.nchunk * P;
    float m = -INFINITY;
    for (int ch = 0; ch < a.nchunk; ++ch) m = fmaxf(m, base[ch * P + q]);
    const float mu = m == -INFINITY ? 0.f : m;
    float l = 0.f, o = 0.f;
    for (int ch = 0; ch < a.nchunk; ++ch) {                     // a chunk whose keys are all masked: f = 0
        const float f = expf(base[ch * P + q] - mu);
        l += base[ch * P + Lq + q] * f;
        o += base[ch * P + 2 * Lq + e] * f;
    }
    a.o[((size_t)b * Lq + q) * a.ldo + h * dh + d] = o / l;    // all keys masked: 0 / 0 = NaN, as in PyTorch
    if (d == 0) a.lse[bh * Lq + q] = m + logf(l);
}

template <int DP>
__global__ __launch_bounds__(256) void mha_splitk_bwd_kernel(const LseArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [16][LD]
    float* dOs = Qs + SKQ * LD;         // [16][LD]
    float* Ks = dOs + SKQ * LD;         // [64][LD]
    float* Vs = Ks + TT * LD;           // [64][LD]
    float* Ps = Vs + TT * LD;           // [4][16 keys][PLD]  P'^T of each wave
    float* Ds = Ps + 4 * SKQ * PLD;     // [4][16 keys][PLD]  dS^T of each wave
    float* rowl = Ds + 4 * SKQ * PLD;   // [16] lse of the queries
    float* rowd = rowl + SKQ;           // [16] delta of the queries
    float* Wa = Ks;                     // after the sweep, over Ks / Vs: [4][16][DP] the waves' dq
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int ch = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int Lq = a.Lq, Lk = a.Lk, dh = a.dh;
    const float* qb = a.q + (size_t)b * Lq * a.ldq + h * dh;
    const float* kb = a.k + (size_t)b * Lk * a.ldk + h * dh;
    const float* vb = a.v + (size_t)b * Lk * a.ldv + h * dh;
    const float* dob = a.d_o + (size_t)b * Lq * a.lddo + h * dh;
    const float* ob = a.o + (size_t)b * Lq * a.ldo + h * dh;
    const size_t bh = (size_t)b * a.heads + h;
    stage_tile<DP, SKQ>(Qs, qb, a.ldq, 0, Lq, dh, tid);
    stage_tile<DP, SKQ>(dOs, dob, a.lddo, 0, Lq, dh, tid);
    if (tid < 4 * SKQ) {                // (wave 0, whole)
        const int q = tid >> 2;
        const float s = sk_delta(dob, a.lddo, ob, a.ldo, q, Lq, dh, tid & 3);
        if ((tid & 3) == 0) {
            rowd[q] = s;
            rowl[q] = q < Lq ? a.lse[bh * Lq + q] : 0.f;
        }
    }
    const int kbeg = ch * a.chunk, kend = min(Lk, kbeg + a.chunk);
    float* Pw = Ps + w * SKQ * PLD;
    float* Dw = Ds + w * SKQ * PLD;
    float* dkb = a.dk + (size_t)b * Lk * a.lddk + h * dh;
    float* dvb = a.dv + (size_t)b * Lk * a.lddv + h * dh;
    f32x4 gq[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) gq[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += TT) {
        __syncthreads();                                        // Q / dO / rowl / rowd staged; the previous tile is done
        stage_tile<DP>(Ks, kb, a.ldk, k0, Lk, dh, tid);
        stage_tile<DP>(Vs, vb, a.ldv, k0, Lk, dh, tid);
        bool live[4];
        uint8_t keepb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = k0 + 16 * w + 4 * kq + r;
            live[r] = !key_masked(a, b, j) && c < Lq;
            keepb[r] = (a.drop && live[r]) ? a.drop[(bh * Lq + c) * Lk + j] : (uint8_t)1;
        }
        __syncthreads();
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
        mma_nt<DP>(s, Ks + 16 * w * LD, Qs, c, kq);             // [key][query]
        mma_nt<DP>(dp, Vs + 16 * w * LD, dOs, c, kq);
        const float li = rowl[c], di = rowd[c];
        float pT[4], dsT[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = live[r] ? expf(s[r] * a.scale - li) : 0.f;
            float keep = 1.f;
            if (a.drop && live[r]) keep = a.drop_scale * (float)keepb[r];
            pT[r] = p * keep;
            dsT[r] = p * (dp[r] * keep - di) * a.scale;
            Pw[(4 * kq + r) * PLD + c] = pT[r];
            Dw[(4 * kq + r) * PLD + c] = dsT[r];
        }
        const float* kp = Ks + (16 * w + 4 * kq) * LD + c;      // dQ[query][d] += dS[query][key] K[key][d], dS from registers
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) gq[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsT[r], kp[r * LD + 16 * n], gq[n], 0, 0, 0);
        __syncthreads();
        // dV[key][d] = P'^T[key][query] dO[query][d], dK[key][d] = dS^T[key][query] Q[query][d]: one 16-deep product each
        const float4 pa = lds4(Pw + c * PLD + 4 * kq), da = lds4(Dw + c * PLD + 4 * kq);
        const float* dop = dOs + 4 * kq * LD + c;
        const float* qp = Qs + 4 * kq * LD + c;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f}, gk = f32x4{0.f, 0.f, 0.f, 0.f};
            gv = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.x, dop[16 * n], gv, 0, 0, 0);
            gv = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.y, dop[LD + 16 * n], gv, 0, 0, 0);
            gv = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.z, dop[2 * LD + 16 * n], gv, 0, 0, 0);
            gv = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.w, dop[3 * LD + 16 * n], gv, 0, 0, 0);
            gk = __builtin_amdgcn_mfma_f32_16x16x4f32(da.x, qp[16 * n], gk, 0, 0, 0);
            gk = __builtin_amdgcn_mfma_f32_16x16x4f32(da.y, qp[LD + 16 * n], gk, 0, 0, 0);
            gk = __builtin_amdgcn_mfma_f32_16x16x4f32(da.z, qp[2 * LD + 16 * n], gk, 0, 0, 0);
            gk = __builtin_amdgcn_mfma_f32_16x16x4f32(da.w, qp[3 * LD + 16 * n], gk, 0, 0, 0);
            if (16 * n + c < dh) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {                   // every key belongs to one tile of one chunk: written once
                    const int j = k0 + 16 * w + 4 * kq + r;
                    if (j < Lk) {
                        dkb[(size_t)j * a.lddk + 16 * n + c] = gk[r];
                        dvb[(size_t)j * a.lddv + 16 * n + c] = gv[r];
                    }
                }
            }
        }
    }
    __syncthreads();
    park_acc<DP>(Wa, gq, w, c, kq);
    __syncthreads();
    float* part = a.ws + (bh * a.nchunk + ch) * (size_t)Lq * dh;      // dq partial [Lq][dh], the waves summed in wave order
    for (int e = tid; e < Lq * dh; e += 256) {
        const int q = e / dh, d = e % dh;
        float g = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) g += Wa[(u * SKQ + q) * DP + d];
        part[e] = g;
    }
}

// dq = the chunks' partials summed in chunk order; block 0 of each (head, clip) also writes delta
__global__ __launch_bounds__(256) void mha_splitk_bwd_reduce_kernel(const LseArgs a) {
    const int Lq = a.Lq, dh = a.dh, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const size_t bh = (size_t)b * a.heads + h;
    if (blockIdx.x == 0 && tid < 4 * SKQ) {                     // (wave 0, whole)
        const int q = tid >> 2;
        const float s = sk_delta(a.d_o + (size_t)b * Lq * a.lddo + h * dh, a.lddo, a.o + (size_t)b * Lq * a.ldo + h * dh,
                                 a.ldo, q, Lq, dh, tid & 3);
        if ((tid & 3) == 0 && q < Lq) a.delta[bh * Lq + q] = s;
    }
    const int e = blockIdx.x * 256 + tid;
    if (e >= Lq * dh) return;
    const size_t P = (size_t)Lq * dh;
    const float* base = a.ws + bh * a.nchunk * P;
    float g = 0.f;
    for (int ch = 0; ch < a.nchunk; ++ch) g += base[ch * P + e];
    a.dq[((size_t)b * Lq + e / dh) * a.lddq + h * dh + e % dh] = g;
}

// The shapes the split-key pair runs: the single statement of its limits (r3d_mha_splitk_supported, and both launches).
static bool splitk_shape_ok(int Lq, int Lk, int dh, bool /*bwd*/) { return Lq >= 1 && Lq <= SKQ && Lk >= 1 && dh >= 1 && dh <= 128; }

// Keys per workgroup: a pure function of (Lk, dh), so a call's bits depend on its arguments alone.
static int splitk_chunk(int /*Lk*/, int /*dh*/) {
    static_assert(R3D_SPLITK_CHUNK > 0 && R3D_SPLITK_CHUNK % TT == 0, "whole 64-key tiles");
    return R3D_SPLITK_CHUNK;
}

static size_t splitk_lds_bytes(int dp, bool bwd) {
    const size_t tiles = (size_t)((bwd ? 2 : 1) * SKQ + 2 * TT) * (dp + 4);
    return (tiles + (bwd ? 2 * 4 * SKQ * PLD + 2 * SKQ : 0)) * sizeof(float);
}

template <int DP>
static int splitk_launch(const LseArgs& a, bool bwd, hipStream_t s) {
    const size_t lds = splitk_lds_bytes(DP, bwd);
    const dim3 gc(a.nchunk, a.heads, a.B), ge(r3d_cdiv(a.Lq * a.dh, 256), a.heads, a.B), blk(256);
    hipError_t e = allow_dynamic_lds(bwd ? (const void*)mha_splitk_bwd_kernel<DP> : (const void*)mha_splitk_fwd_kernel<DP>, lds);
    if (e != hipSuccess) return (int)e;
    if (!bwd) {
        hipLaunchKernelGGL(mha_splitk_fwd_kernel<DP>, gc, blk, lds, s, a);     // chunk partials -> ws ...
        R3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(mha_splitk_fwd_combine_kernel, ge, blk, 0, s, a);   // ... merged into o and lse
        R3D_LAUNCH_CHECK();
        return R3D_OK;
    }
    hipLaunchKernelGGL(mha_splitk_bwd_kernel<DP>, gc, blk, lds, s, a);         // dk, dv; dq partials -> ws ...
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(mha_splitk_bwd_reduce_kernel, ge, blk, 0, s, a);        // ... summed into dq; delta
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

static int splitk_dispatch(LseArgs a, bool bwd, void* stream) {
    int rc = lse_admit(a, splitk_shape_ok(a.Lq, a.Lk, a.dh, bwd), bwd, true);
    if (rc != R3D_OK) return rc;
    a.chunk = splitk_chunk(a.Lk, a.dh);
    a.nchunk = r3d_cdiv(a.Lk, a.chunk);
    hipStream_t s = (hipStream_t)stream;
    switch (tile_dp(a.dh)) {
        case 16: return splitk_launch<16>(a, bwd, s);
        case 32: return splitk_launch<32>(a, bwd, s);
        case 64: return splitk_launch<64>(a, bwd, s);
        default: return splitk_launch<128>(a, bwd, s);
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_mha_splitk_supported(int Lq, int Lk, int dh, int bwd) { return splitk_shape_ok(Lq, Lk, dh, bwd != 0) ? 1 : 0; }

R3D_EXPORT int r3d_mha_splitk_chunk(int Lk, int dh) { return splitk_chunk(Lk, dh); }

R3D_EXPORT size_t r3d_mha_splitk_ws_floats(int B, int heads, int Lq, int Lk, int dh, int bwd) {
    if (B <= 0 || heads <= 0 || !splitk_shape_ok(Lq, Lk, dh, bwd != 0)) return 0;
    const size_t nchunk = (size_t)r3d_cdiv(Lk, splitk_chunk(Lk, dh));
    return (size_t)B * heads * nchunk * Lq * (size_t)(bwd ? dh : dh + 2);
}

R3D_EXPORT int r3d_mha_splitk_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                  const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx,
                                  const uint8_t* drop_mask, float drop_scale, float* o, int ldo, float* lse, float* ws, int B,
                                  int heads, int Lq, int Lk, int dh, void* stream) {
    return splitk_dispatch(lse_args(q, ldq, k, ldk, v, ldv, key_padding_mask, key_label, pad_idx, drop_mask, drop_scale, o, ldo, lse,
                                    nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, ws, B, heads, Lq, Lk, dh),
                           false, stream);
}

R3D_EXPORT int r3d_mha_splitk_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                  const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx,
                                  const uint8_t* drop_mask, float drop_scale, const float* o, int ldo, const float* lse,
                                  const float* d_o, int lddo, float* delta, float* dq, int lddq, float* dk, int lddk, float* dv,
                                  int lddv, float* ws, int B, int heads, int Lq, int Lk, int dh, void* stream) {
    return splitk_dispatch(lse_args(q, ldq, k, ldk, v, ldv, key_padding_mask, key_label, pad_idx, drop_mask, drop_scale, o, ldo, lse,
                                    d_o, lddo, delta, dq, lddq, dk, lddk, dv, lddv, ws, B, heads, Lq, Lk, dh),
                           true, stream);
}
