// The stepwise route of the bidirectional LSTM recurrence: the same layer as csrc/lstm.hip (same tensors, same layouts), for
// hidden sizes whose W_hh no single workgroup can hold (one direction's [4h, h] floats are 1 MiB at hidden 512 and 4 MiB at
// hidden 1024; a CU has 512 KiB of VGPRs).  The weights are spread over the chip instead and every time step is one launch:
// the kernel boundary is the only synchronisation between steps (no flags, no spin loops, no atomics, no cooperative launch),
// and the kernels keep no state of their own between launches: step s reads what step s - 1 wrote into y / cell (forward)
// or dg / the dc carry (backward).
//
// Grid = (tiles of 16 hidden units) x (2 directions) x (tiles of 16 clips), workgroup = 16 waves: 4 gates x 4 slices of the
// contraction.  A workgroup owns 16 units of one direction and all four gates of them.  A step is latency bound (every launch
// finds W_hh outside its L2), so a wave's part of the stream is short enough to be in flight at once: one round trip.
//   forward:  wave (q, ks) takes gate q and slice ks of k: D[unit, clip] = W_hh[q h + unit, k] . h_{t-1}[clip, k] as a chain of
//             fp32-input v_mfma_f32_16x16x4_f32 (slice 0's accumulator starts at gin + b_hh); the 16 partial tiles meet in LDS,
//             and the first 256 threads add the slices in a fixed order, activate the gates and do the cell update of the
//             16 x 16 (unit, clip) pairs.
//   backward: wave (q, ks) takes slice ks of the gate block q of the contraction dh[unit, clip] = sum_j W_hh[j, unit]
//             dG_{t'}[clip, j], reading W_hh from a transposed copy [h, 4h] that one extra launch per layer call makes, so both
//             operands are read as contiguous 64-byte row segments exactly as in the forward; the partial tiles meet in LDS, are
//             added in a fixed order, and the first 256 threads apply the gate adjoints of lstm_bwd_kernel.
// Each lane loads a float4 along the contraction (k = 16 kb + 4 (lane >> 4) + e feeds MFMA e of block kb, for both operands),
// so the order of the sum is fixed and the same call gives the same bits.  h % 4 == 0 (hidden % 8 == 0), so a float4 is wholly
// inside or wholly outside every bound: tails of units, of the contraction and of clips are predicated loads of zeros.
#include "common.h"
#include "../../include/r3d_hip.h"

namespace r3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepUnits = 16, kStepClips = 16, kStepSlices = 4, kStepThreads = 64 * 4 * kStepSlices;

__device__ __forceinline__ float lstm_step_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct LstmStepFwdArgs {
    const float* gin; int ldgin;
    const float* whh0; const float* whh1;  // [4h, h] per direction
    const float* bhh0; const float* bhh1;
    float* y; int ldy;
    float* gates; int ldgates;
    float* cell; int ldcell;
    float* hprev; int ldhprev;
    int B, S, h;
};

struct LstmStepBwdArgs {
    const float* dy; int lddy;
    const float* wt;                       // [2][h][4h]: W_hh of each direction, transposed
    const float* gates; int ldgates;
    const float* cell; int ldcell;
    float* dg; int lddg;
    float* dc;                             // [B, 2h]: dL/dc carried from one backward step to the next
    int B, S, h;
};

__device__ __forceinline__ float4 ld4_or_zero(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// acc[r] += sum over k in [k_lo, k_hi) of A[lane & 15][k] Bm[lane & 15][k] in the 16x16x4 C/D layout (row 4 (lane >> 4) + r of
// A, column lane & 15 of Bm); arow / brow: this lane's rows, K floats long (K % 4 == 0), read only where aok / bok and k < K.
// Two accumulators, even and odd 16-blocks of k, added at the end.
__device__ __forceinline__ f32x4 tile_dot16(const float* arow, bool aok, const float* brow, bool bok, int K, int k_lo, int k_hi,
                                            int g4, f32x4 acc0) {
    f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = k_lo; k0 < k_hi; k0 += 32) {
        const int ka = k0 + g4, kb = k0 + 16 + g4;
        const float4 a0 = ld4_or_zero(arow + ka, aok && ka < K), b0 = ld4_or_zero(brow + ka, bok && ka < K);
        const float4 a1 = ld4_or_zero(arow + kb, aok && kb < K), b1 = ld4_or_zero(brow + kb, bok && kb < K);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// the contraction range of slice ks of kStepSlices: whole 32-blocks of k, the same count for every slice
__device__ __forceinline__ void slice_range(int K, int ks, int& k_lo, int& k_hi) {
    const int per = ((K + 31) / 32 + kStepSlices - 1) / kStepSlices * 32;
    k_lo = ks * per;
    k_hi = min(K, k_lo + per);
}

__global__ __launch_bounds__(kStepThreads) void lstm_step_fwd_kernel(const LstmStepFwdArgs a, const int step) {
    __shared__ float part[kStepSlices][4][kStepUnits][kStepClips + 1];    // [k slice][gate][unit][clip]
    const int h = a.h, G = 4 * h, S = a.S;
    const int u0 = (int)blockIdx.x * kStepUnits, d = (int)blockIdx.y, b0 = (int)blockIdx.z * kStepClips;
    const int tid = (int)threadIdx.x, wv = tid >> 6, q = wv & 3, ks = wv >> 2, lane = tid & 63;
    const int t = d ? S - 1 - step : step;
    const int tp = d ? t + 1 : t - 1;                         // the direction's previous frame (step > 0)
    const size_t hcol = (size_t)d * h;
    // the cell update's operands of this thread's (unit, clip) pair, loaded under the products
    const int ui = u0 + (tid & 15), bi = b0 + ((tid >> 4) & 15);
    const bool pair = tid < kStepUnits * kStepClips && ui < h && bi < a.B;
    float hp = 0.f, cp = 0.f;
    if (pair && step > 0) {
        const size_t prow = (size_t)bi * S + tp;
        hp = a.y[prow * a.ldy + hcol + ui];
        cp = a.cell[prow * a.ldcell + hcol + ui];
    }
    {
        const int li = lane & 15, g4 = 4 * (lane >> 4);
        const int ua = u0 + li, bj = b0 + li, uc = u0 + g4;   // A row; B row = C/D column; first of this lane's 4 C/D rows
        const bool aok = ua < h, bok = bj < a.B;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (ks == 0 && bok && uc < h) {                       // slice 0's chain starts at gin + b_hh
            const float4 gi = *reinterpret_cast<const float4*>(a.gin + ((size_t)bj * S + t) * a.ldgin + (size_t)d * G +
                                                               (size_t)q * h + uc);
            const float4 bb = *reinterpret_cast<const float4*>((d ? a.bhh1 : a.bhh0) + q * h + uc);
            acc[0] = gi.x + bb.x; acc[1] = gi.y + bb.y; acc[2] = gi.z + bb.z; acc[3] = gi.w + bb.w;
        }
        if (step > 0) {
            const float* W = d ? a.whh1 : a.whh0;
            const float* arow = W + (size_t)(q * h + (aok ? ua : 0)) * h;
            const float* brow = a.y + ((size_t)(bok ? bj : 0) * S + tp) * a.ldy + hcol;
            int k_lo, k_hi;
            slice_range(h, ks, k_lo, k_hi);
            acc = tile_dot16(arow, aok, brow, bok, h, k_lo, k_hi, g4, acc);
        }
        part[ks][q][g4 + 0][li] = acc[0]; part[ks][q][g4 + 1][li] = acc[1];
        part[ks][q][g4 + 2][li] = acc[2]; part[ks][q][g4 + 3][li] = acc[3];
    }
    __syncthreads();
    if (pair) {
        const int i = tid & 15, j = tid >> 4;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = (part[0][g][i][j] + part[1][g][i][j]) + (part[2][g][i][j] + part[3][g][i][j]);
        const float ig = lstm_step_sigmoid(pre[0]), fg = lstm_step_sigmoid(pre[1]), gg = tanhf(pre[2]),
                    og = lstm_step_sigmoid(pre[3]);
        const float c = fg * cp + ig * gg;
        const float hn = og * tanhf(c);
        const size_t row = (size_t)bi * S + t;
        float* gr = a.gates + row * a.ldgates + (size_t)d * G + ui;
        gr[0] = ig; gr[h] = fg; gr[2 * h] = gg; gr[3 * h] = og;
        a.hprev[row * a.ldhprev + hcol + ui] = hp;
        a.cell[row * a.ldcell + hcol + ui] = c;
        a.y[row * a.ldy + hcol + ui] = hn;
    }
}

__global__ __launch_bounds__(kStepThreads) void lstm_step_bwd_kernel(const LstmStepBwdArgs a, const int s) {
    __shared__ float part[kStepSlices][4][kStepUnits][kStepClips + 1];    // [k slice][gate block of the contraction][unit][clip]
    const int h = a.h, G = 4 * h, S = a.S;
    const int u0 = (int)blockIdx.x * kStepUnits, d = (int)blockIdx.y, b0 = (int)blockIdx.z * kStepClips;
    const int tid = (int)threadIdx.x, wv = tid >> 6, q = wv & 3, ks = wv >> 2, lane = tid & 63;
    const int tau = S - 1 - s;                                // the direction's processing step
    const int t = d ? S - 1 - tau : tau;
    const int tn = d ? t - 1 : t + 1;                         // the frame the previous backward launch wrote (s > 0)
    const int tp = d ? t + 1 : t - 1;                         // the direction's previous frame (tau > 0)
    const size_t gcol = (size_t)d * G, hcol = (size_t)d * h;
    const int ui = u0 + (tid & 15), bi = b0 + ((tid >> 4) & 15);
    const bool pair = tid < kStepUnits * kStepClips && ui < h && bi < a.B;
    float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cc = 0.f, cp = 0.f, dyv = 0.f, dc = 0.f;
    if (pair) {
        const size_t row = (size_t)bi * S + t;
        const float* gr = a.gates + row * a.ldgates + gcol + ui;
        ig = gr[0]; fg = gr[h]; gg = gr[2 * h]; og = gr[3 * h];
        cc = a.cell[row * a.ldcell + hcol + ui];
        if (tau > 0) cp = a.cell[((size_t)bi * S + tp) * a.ldcell + hcol + ui];
        dyv = a.dy[row * a.lddy + hcol + ui];
        if (s > 0) dc = a.dc[(size_t)bi * 2 * h + hcol + ui];
    }
    {
        const int li = lane & 15, g4 = 4 * (lane >> 4);
        const int ua = u0 + li, bj = b0 + li;
        const bool aok = ua < h, bok = bj < a.B;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            const float* arow = a.wt + ((size_t)d * h + (aok ? ua : 0)) * G + (size_t)q * h;
            const float* brow = a.dg + ((size_t)(bok ? bj : 0) * S + tn) * a.lddg + gcol + (size_t)q * h;
            int k_lo, k_hi;
            slice_range(h, ks, k_lo, k_hi);
            acc = tile_dot16(arow, aok, brow, bok, h, k_lo, k_hi, g4, acc);
        }
        part[ks][q][g4 + 0][li] = acc[0]; part[ks][q][g4 + 1][li] = acc[1];
        part[ks][q][g4 + 2][li] = acc[2]; part[ks][q][g4 + 3][li] = acc[3];
    }
    __syncthreads();
    if (pair) {
        const int i = tid & 15, j = tid >> 4;
        float sq[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) sq[g] = (part[0][g][i][j] + part[1][g][i][j]) + (part[2][g][i][j] + part[3][g][i][j]);
        const float dh = dyv + ((sq[0] + sq[1]) + (sq[2] + sq[3]));
        const float tc = tanhf(cc);
        const float dct = dc + dh * og * (1.f - tc * tc);
        const float dgi = dct * gg * ig * (1.f - ig);
        const float dgf = dct * cp * fg * (1.f - fg);
        const float dgg = dct * ig * (1.f - gg * gg);
        const float dgo = dh * tc * og * (1.f - og);
        float* o = a.dg + ((size_t)bi * S + t) * a.lddg + gcol + ui;
        o[0] = dgi; o[h] = dgf; o[2 * h] = dgg; o[3 * h] = dgo;
        a.dc[(size_t)bi * 2 * h + hcol + ui] = dct * fg;
    }
}

// wt[d][m][j] = W_hh(d)[j][m]: 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void lstm_step_transpose_kernel(const float* w0, const float* w1, float* wt, int h) {
    __shared__ float tile[32][33];
    const int G = 4 * h, d = (int)blockIdx.z;
    const float* W = d ? w1 : w0;
    float* out = wt + (size_t)d * h * G;
    const int j0 = (int)blockIdx.x * 32, m0 = (int)blockIdx.y * 32;
    const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, m = m0 + tx;
        tile[r][tx] = (j < G && m < h) ? W[(size_t)j * h + m] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r, j = j0 + tx;
        if (m < h && j < G) out[(size_t)m * G + j] = tile[tx][r];
    }
}

static bool steps_shape_ok(int B, int S, int H) {
    return B > 0 && S > 0 && r3d_lstm_steps_supported(H) && r3d_cdiv(B, kStepClips) <= 65535;
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_lstm_steps_supported(int H) { return (H >= 8 && H <= 1024 && H % 8 == 0) ? 1 : 0; }

R3D_EXPORT int64_t r3d_lstm_steps_ws_floats(int B, int H) {
    if (B <= 0 || !r3d_lstm_steps_supported(H)) return R3D_EINVAL;
    return (int64_t)B * H + (int64_t)2 * H * H;               // dc carry [B, 2h] + the transposed W_hh [2][h][4h]
}

R3D_EXPORT int r3d_lstm_steps_layer_fwd(const float* gin, int ldgin, const float* whh_fwd, const float* whh_rev,
                                        const float* bhh_fwd, const float* bhh_rev, float* y, int ldy, float* gates, int ldgates,
                                        float* cell, int ldcell, float* hprev, int ldhprev, int B, int S, int H, void* stream) {
    R3D_REQUIRE(gin && whh_fwd && whh_rev && bhh_fwd && bhh_rev && y && gates && cell && hprev);
    R3D_REQUIRE(steps_shape_ok(B, S, H));
    const int h = H / 2;
    R3D_REQUIRE(ldgin >= 8 * h && ldgates >= 8 * h && ldy >= 2 * h && ldcell >= 2 * h && ldhprev >= 2 * h);
    if (!(r3d_aligned16(gin) && r3d_aligned16(whh_fwd) && r3d_aligned16(whh_rev) && r3d_aligned16(bhh_fwd) &&
          r3d_aligned16(bhh_rev) && r3d_aligned16(y) && r3d_aligned16(gates)) || ldgin % 4 || ldy % 4 || ldgates % 4)
        return R3D_EALIGN;
    const LstmStepFwdArgs a{gin, ldgin, whh_fwd, whh_rev, bhh_fwd, bhh_rev, y, ldy, gates, ldgates, cell, ldcell, hprev,
                            ldhprev, B, S, h};
    const dim3 grid(r3d_cdiv(h, kStepUnits), 2, r3d_cdiv(B, kStepClips)), block(kStepThreads);
    for (int step = 0; step < S; ++step) {
        hipLaunchKernelGGL(lstm_step_fwd_kernel, grid, block, 0, (hipStream_t)stream, a, step);
        R3D_LAUNCH_CHECK();
    }
    return R3D_OK;
}

R3D_EXPORT int r3d_lstm_steps_layer_bwd(const float* dy, int lddy, const float* whh_fwd, const float* whh_rev, const float* gates,
                                        int ldgates, const float* cell, int ldcell, float* dg, int lddg, int B, int S, int H,
                                        float* ws, void* stream) {
    R3D_REQUIRE(dy && whh_fwd && whh_rev && gates && cell && dg && ws);
    R3D_REQUIRE(steps_shape_ok(B, S, H));
    const int h = H / 2;
    R3D_REQUIRE(lddy >= 2 * h && ldgates >= 8 * h && ldcell >= 2 * h && lddg >= 8 * h);
    if (!(r3d_aligned16(dg) && r3d_aligned16(ws)) || lddg % 4) return R3D_EALIGN;
    float* dc = ws;
    float* wt = ws + (size_t)B * H;                           // (B H floats: a multiple of 8, so wt stays 16-byte aligned)
    const LstmStepBwdArgs a{dy, lddy, wt, gates, ldgates, cell, ldcell, dg, lddg, dc, B, S, h};
    if (S > 1) {                                              // (a single step has no recurrent term: nothing reads wt)
        const dim3 tgrid(r3d_cdiv(4 * h, 32), r3d_cdiv(h, 32), 2);
        hipLaunchKernelGGL(lstm_step_transpose_kernel, tgrid, dim3(256), 0, (hipStream_t)stream, whh_fwd, whh_rev, wt, h);
        R3D_LAUNCH_CHECK();
    }
    const dim3 grid(r3d_cdiv(h, kStepUnits), 2, r3d_cdiv(B, kStepClips)), block(kStepThreads);
    for (int s = 0; s < S; ++s) {
        hipLaunchKernelGGL(lstm_step_bwd_kernel, grid, block, 0, (hipStream_t)stream, a, s);
        R3D_LAUNCH_CHECK();
    }
    return R3D_OK;
}
