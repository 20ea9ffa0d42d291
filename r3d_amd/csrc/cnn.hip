// The segmentation-head step of the CNN baseline (reference model/cnn.py: seg = fc_seg(x) on the S frames of every clip,
// x = relu(input_embed(features))) as ONE row-tile launch: logits, the per-row cross entropy unit, d_seg, d_seg . W and
// the ReLU gate into the embedding's pre-activation gradient,
//
//   logits = x . W^T + b                                   [N, Kseg]     (stored to `seg` when that pointer is not null)
//   unit r = { loss term, correct, valid }                               (the segmentation unit of losses_unit, losses_dev.h:
//                                                                         masked when the label is pad_idx, exclude_idx or
//                                                                         outside [0, Kseg); + 2 when the arg-max is pad_idx)
//   d_seg  = (softmax(logits) - onehot) grad_scale / N     [N, Kseg]     zero on masked rows
//   d_pre  = (x > 0) ? d_seg . W + d_x0 + d_extra : 0      [N, H]
//
// Tile discipline of supcon.hip / attention_tiled.hip (tile_mma.h): grid ceil(N / 64) over the frame ROWS (not clips), 256
// threads, the tile's 64 rows of x staged once with the width zero-padded to DP in {16, 32, 64, 128, 256}, the weight
// streamed in chunks of 64 classes, 64 x 64 score tiles, fp32-input MFMA chains.  x tile + weight chunk + score tile are
// 150 KiB of LDS at DP = 256.
//
//   sweep 1   per chunk: logits -> score tile (and `seg`); per row the running maximum, the sum of exponentials under it (in double),
//             the arg-max (first occurrence of the largest value, the rule of ce_row) and the label's logit.
//   row       lse = max + log(sum); the unit goes to ws in r3d_losses_fwd_bwd's layout (unit r of the [B S | B Q | B] grid)
//             with the same agent-scope stores, so r3d_losses_finalize or the AdamW rider reduces it with has_seg = 1.
//   sweep 2   per chunk: the logits again, d_logit -> score tile and d_seg, d_x += d_logit . W_chunk in registers.
//   epilogue  d_x waits in the weight chunk's LDS, then d_pre leaves in 16-byte rows next to d_x0 / d_extra.
//
// No atomics, every sum in a fixed order: the same call gives the same bits.
#include "common.h"
#include "tile_mma.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int kCnnMaxH = 256;           // the widest DP of tile_mma.h
constexpr int kCnnMaxK = 1023;
constexpr int kCnnMaxRows = 1 << 28;    // row and unit indices stay in int

struct CnnLds {
    float *X, *Wc, *Ss, *lse, *scale;
    int* lab;
};

template <int DP>
__device__ __forceinline__ CnnLds cnn_lds(float* lds) {
    constexpr int LD = DP + 4;
    CnnLds s;
    s.X = lds;                          // [64][LD] the tile's rows of x
    s.Wc = s.X + TT * LD;               // [64][LD] 64 classes of fc_seg.weight; in the epilogue the tile's d_x
    s.Ss = s.Wc + TT * LD;              // [64][SLD] logits, then d_logit
    s.lse = s.Ss + TT * SLD;            // [64] per row: log-sum-exp, grad_scale / N (0 on a masked row), label (-1 on one)
    s.scale = s.lse + TT;
    s.lab = reinterpret_cast<int*>(s.scale + TT);
    return s;
}

static size_t cnn_lds_bytes(int dp) { return ((size_t)2 * TT * (dp + 4) + (size_t)TT * SLD + 3 * TT) * sizeof(float); }

// logits of the tile's rows against the staged chunk: wave w's 16 rows x 64 classes, bias added
template <int DP>
__device__ __forceinline__ void cnn_logits(const CnnLds& s, const r3d_cnn_seg_args& a, int k0, int w, int c, int kq, f32x4 (&sc)[4]) {
    constexpr int LD = DP + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        mma_nt<DP>(sc[t], s.X + 16 * w * LD, s.Wc + 16 * t * LD, c, kq);
        const int k = k0 + 16 * t + c;
        const float bias = k < a.Kseg ? a.b[k] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] += bias;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void cnn_seg_step_kernel(const r3d_cnn_seg_args a, float* part) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const CnnLds s = cnn_lds<DP>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int N = a.N, H = a.H, K = a.Kseg, i0 = blockIdx.x * TT;
    // statistics role: row srow of the tile, columns 4 t + part
    const int srow = 16 * w + (lane >> 2), part_l = lane & 3, gi = i0 + srow;
    stage_tile<DP>(s.X, a.x, a.ld_x, i0, N, H, tid);
    const int64_t lab = gi < N ? a.labels[gi] : (int64_t)-1;
    const bool valid = gi < N && lab != (int64_t)a.pad_idx && lab != (int64_t)a.exclude_idx && lab >= 0 && lab < (int64_t)K;
    // ---- sweep 1
    // the sum of exponentials and its logarithm in double: the row's loss is then as exact as its float32 logits allow (in
    // float32 the rounding of lse = max + log(sum) alone is an ulp of lse, which a small loss does not hide)
    float m = -INFINITY, lab_logit = 0.f;
    double l = 0.0;
    int am = 0x7fffffff;
    for (int k0 = 0; k0 < K; k0 += TT) {
        __syncthreads();                                        // the previous chunk's readers are done with Wc / Ss
        stage_tile<DP>(s.Wc, a.w, H, k0, K, H, tid);
        __syncthreads();
        f32x4 sc[4];
        cnn_logits<DP>(s, a, k0, w, c, kq, sc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 16 * t + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                s.Ss[row * SLD + col] = sc[t][r];
                if (a.seg && i0 + row < N && k0 + col < K) a.seg[(size_t)(i0 + row) * a.ld_seg + k0 + col] = sc[t][r];
            }
        }
        __syncthreads();
        float sv[16], mx = -INFINITY;
        int ax = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = 4 * t + part_l;
            sv[t] = s.Ss[srow * SLD + col];
            if (k0 + col < K && sv[t] > mx) { mx = sv[t]; ax = k0 + col; }       // ascending columns: the lane's first occurrence
        }
#pragma unroll
        for (int off = 1; off <= 2; off <<= 1) {
            const float om = __shfl_xor(mx, off);
            const int oa = __shfl_xor(ax, off);
            if (om > mx || (om == mx && oa < ax)) { mx = om; ax = oa; }
        }
        if (mx > m) am = ax;                                    // (strictly: an earlier chunk keeps a tie)
        const float m_new = fmaxf(m, mx);
        double sum = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int k = k0 + 4 * t + part_l;
            if (k >= K) continue;
            sum += exp((double)sv[t] - (double)m_new);
            if ((int64_t)k == lab) lab_logit += sv[t];
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        l = l * exp((double)m - (double)m_new) + sum;
        m = m_new;
    }
    lab_logit = quad_sum(lab_logit);
    const double log_l = log(l);
    const float lse = (float)((double)m + log_l);
    if (part_l == 0) {
        s.lse[srow] = lse;
        s.scale[srow] = valid ? a.grad_scale / (float)N : 0.f;
        s.lab[srow] = valid ? (int)lab : -1;
        if (gi < N) {
            float out_l = valid ? (float)(((double)m - (double)lab_logit) + log_l) : 0.f;
            if (valid && am == a.pad_idx) out_l += 2.0f;        // penalty term of cal_loss, as in losses_unit
            const float out_c = (valid && (int64_t)am == lab) ? 1.f : 0.f, out_v = valid ? 1.f : 0.f;
            __hip_atomic_store(part + 4 * (size_t)gi + 0, out_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part + 4 * (size_t)gi + 1, out_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part + 4 * (size_t)gi + 2, out_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- sweep 2
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += TT) {
        __syncthreads();                                        // row statistics written; the previous chunk's readers are done
        stage_tile<DP>(s.Wc, a.w, H, k0, K, H, tid);
        __syncthreads();
        f32x4 sc[4];
        cnn_logits<DP>(s, a, k0, w, c, kq, sc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 16 * t + c, k = k0 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                const float scl = s.scale[row];
                float g = 0.f;
                if (k < K && scl != 0.f) g = (expf(sc[t][r] - s.lse[row]) - (k == s.lab[row] ? 1.f : 0.f)) * scl;
                s.Ss[row * SLD + col] = g;
                if (i0 + row < N && k < K) a.d_seg[(size_t)(i0 + row) * a.ld_dseg + k] = g;
            }
        }
        __syncthreads();
        mma_nn<DP>(acc, s.Ss + 16 * w * SLD, s.Wc, c, kq);
    }
    // ---- epilogue: d_x through the weight chunk's LDS, then the gate in 16-byte rows
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) s.Wc[(16 * w + 4 * kq + r) * LD + 16 * n + c] = acc[n][r];
    __syncthreads();
    for (int e = tid; e < TT * DP / 4; e += 256) {
        const int r = e / (DP / 4), d = (e % (DP / 4)) * 4;
        if (i0 + r >= N || d >= H) continue;
        const size_t row = (size_t)(i0 + r);
        const float4 x = lds4(s.X + r * LD + d);
        float4 g = lds4(s.Wc + r * LD + d);
        if (a.d_x0) {
            const float4 v = *reinterpret_cast<const float4*>(a.d_x0 + row * a.ld_dx0 + d);
            g.x += v.x; g.y += v.y; g.z += v.z; g.w += v.w;
        }
        if (a.d_extra) {
            const float4 v = *reinterpret_cast<const float4*>(a.d_extra + row * a.ld_dextra + d);
            g.x += v.x; g.y += v.y; g.z += v.z; g.w += v.w;
        }
        g.x = x.x > 0.f ? g.x : 0.f; g.y = x.y > 0.f ? g.y : 0.f; g.z = x.z > 0.f ? g.z : 0.f; g.w = x.w > 0.f ? g.w : 0.f;
        *reinterpret_cast<float4*>(a.d_pre + row * a.ld_dpre + d) = g;
    }
}

// The shapes the kernel runs: the single statement of its limit (r3d_cnn_seg_supported, and the launch).
static bool cnn_shape_ok(int H, int Kseg) { return H >= 8 && H % 4 == 0 && H <= kCnnMaxH && Kseg >= 1 && Kseg <= kCnnMaxK; }

template <int DP>
static int cnn_launch(const r3d_cnn_seg_args& a, float* ws, hipStream_t s) {
    const size_t lds = cnn_lds_bytes(DP);
    hipError_t e = allow_dynamic_lds((const void*)cnn_seg_step_kernel<DP>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cnn_seg_step_kernel<DP>, dim3(r3d_cdiv(a.N, TT)), dim3(256), lds, s, a, ws);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

}  // namespace r3d

using namespace r3d;

/* 1: the segmentation-head step takes hidden H and Kseg classes (host-only): H % 4 == 0, 8 <= H <= 256, 1 <= Kseg <= 1023. */
R3D_EXPORT int r3d_cnn_seg_supported(int H, int Kseg) { return cnn_shape_ok(H, Kseg) ? 1 : 0; }

R3D_EXPORT int r3d_cnn_seg_step(const r3d_cnn_seg_args* p, float* ws, void* stream) {
    R3D_REQUIRE(p && ws);
    const r3d_cnn_seg_args& a = *p;
    if (!cnn_shape_ok(a.H, a.Kseg)) return R3D_EINVAL;
    R3D_REQUIRE(a.x && a.w && a.b && a.labels && a.d_seg && a.d_pre);
    R3D_REQUIRE(a.N >= 1 && a.N <= kCnnMaxRows && a.ld_x >= a.H && a.ld_dseg >= a.Kseg && a.ld_dpre >= a.H);
    R3D_REQUIRE(!a.seg || a.ld_seg >= a.Kseg);
    R3D_REQUIRE(!a.d_x0 || a.ld_dx0 >= a.H);
    R3D_REQUIRE(!a.d_extra || a.ld_dextra >= a.H);
    if (!r3d_aligned16(a.x) || !r3d_aligned16(a.w) || !r3d_aligned16(a.d_pre) || !r3d_aligned16(a.d_x0) ||
        !r3d_aligned16(a.d_extra) || !r3d_aligned16(ws) || a.ld_x % 4 || a.ld_dpre % 4 || (a.d_x0 && a.ld_dx0 % 4) ||
        (a.d_extra && a.ld_dextra % 4))
        return R3D_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    switch (tile_dp(a.H)) {
        case 16: return cnn_launch<16>(a, ws, s);
        case 32: return cnn_launch<32>(a, ws, s);
        case 64: return cnn_launch<64>(a, ws, s);
        case 128: return cnn_launch<128>(a, ws, s);
        default: return cnn_launch<256>(a, ws, s);
    }
}
