// The pooled-head chain of the AFFT baseline (model/afft.py of the reference, :189-201): everything behind the fused tokens
// is local to one clip,
//   pooled = adaptive_avg_pool1d(fused, Q)   [Q, H]      windows of pool_dev.h; they overlap by one frame when S % Q != 0 and
//                                                        repeat frames when S < Q; padded frames are pooled like any other
//   actdur = pooled . w_head^T + b_head      [Q, K + 1]  fc and fc_len as one [K + 1, H] weight, duration in column K
// so ONE workgroup per clip runs it: r3d_afft_head_fwd the two lines above, r3d_afft_head_step in addition the clip's
// anticipation CE rows and its duration unit (losses_unit of losses_dev.h, the arithmetic of r3d_losses_fwd_bwd), the
// heads' input gradient d_pooled = d_actdur . w_head and the pool's adjoint in gather form (frame s sums d_pooled[q] / len_q
// over every window that contains it, ascending q).  No atomics, every sum in a fixed order: the same call gives the same
// bits.  The pooled rows (then their gradients) and d_actdur wait in LDS; w_head is streamed through L2 (every clip reads
// the same <= 124 x 1024 floats), never staged whole.
//
// Loss partials: the layout of r3d_losses_fwd_bwd, [B S | B Q | B] units of 4 floats.  The model has no 'seg' output: each
// clip's workgroup writes zeros into its S segmentation units (the reduction adds their counters whatever has_seg says, so
// nothing an earlier user of the scratch left there may survive), and the reduction runs with has_seg = 0 --
// r3d_losses_finalize, or the AdamW launch's extra workgroup.  The step counter and the dropout offset tick here
// (workgroup 0), as in the deferred form of r3d_decoder_tail_losses.
#include "losses_dev.h"
#include "pool_dev.h"

namespace r3d {

constexpr int kAfftThreads = 1024;           // 16 waves per clip: head rows, loss units and pooled columns side by side
constexpr int kAfftWaves = kAfftThreads / 64;
constexpr int kAfftMaxH = 1024;              // a head weight row in one wave's registers: 16 floats per lane
constexpr int kAfftMaxQ = 64;
constexpr int kAfftMaxHeads = 1024;
constexpr size_t kAfftMaxLds = 152 * 1024;   // of the CU's 160 KiB

// win[2 q], win[2 q + 1] = window of output q (pool_dev.h), once per workgroup: the gather asks for every window of every frame
__device__ __forceinline__ void afft_windows(const r3d_afft_head_args& a, int* win) {
    if ((int)threadIdx.x < a.Q) {
        win[2 * threadIdx.x] = pool_start(threadIdx.x, a.S, a.Q);
        win[2 * threadIdx.x + 1] = pool_end(threadIdx.x, a.S, a.Q);
    }
}

// pooled rows of clip b -> LDS pl [Q][H] and global a.pooled; sequential sum over the window, then / len (= avgpool_fwd_kernel).
// One thread per column while that keeps the workgroup busy, four columns per thread beyond: the same sums either way.
__device__ __forceinline__ void afft_pool(const r3d_afft_head_args& a, int b, float* pl, const int* win) {
    if (a.Q * a.H <= 2 * kAfftThreads) {
        for (int i = threadIdx.x; i < a.Q * a.H; i += kAfftThreads) {
            const int q = i / a.H, c = i - q * a.H;
            const int s0 = win[2 * q], s1 = win[2 * q + 1];
            float acc = 0.f;
            const float* src = a.fused + ((size_t)b * a.S + s0) * a.ld_fused + c;
#pragma unroll 8
            for (int s = s0; s < s1; ++s, src += a.ld_fused) acc += *src;
            acc /= (float)(s1 - s0);
            pl[i] = acc;
            a.pooled[((size_t)b * a.Q + q) * a.H + c] = acc;
        }
        return;
    }
    const int H4 = a.H >> 2;
    for (int i = threadIdx.x; i < a.Q * H4; i += kAfftThreads) {
        const int q = i / H4, c = (i - q * H4) << 2;
        const int s0 = win[2 * q], s1 = win[2 * q + 1];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* src = a.fused + ((size_t)b * a.S + s0) * a.ld_fused + c;
#pragma unroll 4
        for (int s = s0; s < s1; ++s, src += a.ld_fused) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const float len = (float)(s1 - s0);
        acc.x /= len; acc.y /= len; acc.z /= len; acc.w /= len;
        *reinterpret_cast<float4*>(pl + (size_t)q * a.H + c) = acc;
        *reinterpret_cast<float4*>(a.pooled + ((size_t)b * a.Q + q) * a.H + c) = acc;
    }
}

// actdur[q][k] = pooled[q] . w_head[k] + b_head[k]: wave w takes the head rows k = w, w + 16, ..., keeps the row in registers
// and walks the clip's Q pooled rows in LDS
__device__ __forceinline__ void afft_heads(const r3d_afft_head_args& a, int b, const float* pl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < a.n_head; k += kAfftWaves) {
        float w[kAfftMaxH / 64];
#pragma unroll
        for (int e = 0; e < kAfftMaxH / 64; ++e) {
            const int c = lane + 64 * e;
            w[e] = c < a.H ? a.w_head[(size_t)k * a.H + c] : 0.f;
        }
        const float bias = a.b_head[k];
        for (int q = 0; q < a.Q; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < kAfftMaxH / 64; ++e) {
                const int c = lane + 64 * e;
                if (c < a.H) acc += w[e] * pl[(size_t)q * a.H + c];
            }
            acc = wave_sum(acc);
            if (lane == 0) a.out[((size_t)b * a.Q + q) * a.ld_out + k] = acc + bias;
        }
    }
}

__global__ __launch_bounds__(kAfftThreads) void afft_head_fwd_kernel(const r3d_afft_head_args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int win[2 * kAfftMaxQ];
    const int b = blockIdx.x;
    afft_windows(a, win);
    __syncthreads();
    afft_pool(a, b, lds, win);
    __syncthreads();
    afft_heads(a, b, lds);
}

__global__ __launch_bounds__(kAfftThreads) void afft_head_step_kernel(const r3d_afft_head_args a, const LossArgs la, float* part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int win[2 * kAfftMaxQ];
    float* pl = lds;                                  // [Q][H] pooled rows, later their gradients
    float* ad = lds + (size_t)a.Q * a.H;              // [Q][K + 1] d_actdur
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.B * a.S, BQ = a.B * a.Q, NH = a.n_head;
    afft_windows(a, win);
    // the clip's S segmentation units: this model has none, and the reduction must not meet what an earlier user of the
    // scratch left there
    for (int i = threadIdx.x; i < 4 * a.S; i += kAfftThreads) part[4 * (size_t)b * a.S + i] = 0.f;
    __syncthreads();
    afft_pool(a, b, pl, win);
    __syncthreads();
    afft_heads(a, b, pl);
    __syncthreads();                                  // the clip's logits are in memory (this workgroup wrote them)
    // ---- the clip's Q anticipation rows and its duration unit, a wave each: d_actdur rows of the clip, loss partials
    if (wave == kAfftWaves - 1) losses_unit(la, part, N + BQ + b, lane);
    for (int q = wave; q < a.Q; q += kAfftWaves) losses_unit(la, part, N + b * a.Q + q, lane);
    // losses_unit left d_actdur in global memory (the weight-gradient launch reads it there); this workgroup reads its own rows
    // back into LDS, relying on __syncthreads ordering a workgroup's global stores before its later loads (as above for `out`)
    __syncthreads();
    for (int i = threadIdx.x; i < a.Q * NH; i += kAfftThreads) {
        const int q = i / NH, k = i - q * NH;
        ad[i] = a.d_out[((size_t)b * a.Q + q) * a.ld_dout + k];
    }
    __syncthreads();
    // ---- d_pooled[q] = sum_k d_actdur[q][k] w_head[k], ascending k (one column per thread while that keeps the workgroup busy)
    const int H4 = a.H >> 2;
    if (a.Q * a.H <= 2 * kAfftThreads) {
        for (int i = threadIdx.x; i < a.Q * a.H; i += kAfftThreads) {
            const int q = i / a.H, c = i - q * a.H;
            float acc = 0.f;
            const float* wp = a.w_head + c;
#pragma unroll 8
            for (int k = 0; k < NH; ++k, wp += a.H) acc += ad[q * NH + k] * *wp;
            pl[i] = acc;
        }
    } else {
        for (int i = threadIdx.x; i < a.Q * H4; i += kAfftThreads) {
            const int q = i / H4, c = (i - q * H4) << 2;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* wp = a.w_head + c;
#pragma unroll 4
            for (int k = 0; k < NH; ++k, wp += a.H) {
                const float g = ad[q * NH + k];
                const float4 w = *reinterpret_cast<const float4*>(wp);
                acc.x += g * w.x; acc.y += g * w.y; acc.z += g * w.z; acc.w += g * w.w;
            }
            *reinterpret_cast<float4*>(pl + (size_t)q * a.H + c) = acc;
        }
    }
    __syncthreads();
    // ---- d_fused[s] = sum over the windows that contain s of d_pooled[q] / len_q, ascending q (= avgpool_bwd_kernel)
    for (int i = threadIdx.x; i < a.S * H4; i += kAfftThreads) {
        const int s = i / H4, c = (i - s * H4) << 2;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = 0; q < a.Q; ++q) {
            const int s0 = win[2 * q], s1 = win[2 * q + 1];
            if (s >= s0 && s < s1) {
                const float len = (float)(s1 - s0);
                const float4 g = *reinterpret_cast<const float4*>(pl + (size_t)q * a.H + c);
                acc.x += g.x / len; acc.y += g.y / len; acc.z += g.z / len; acc.w += g.w / len;
            }
        }
        float4* dst = reinterpret_cast<float4*>(a.d_fused + ((size_t)b * a.S + s) * a.ld_dfused + c);
        float4 o = make_float4(a.gscale * acc.x, a.gscale * acc.y, a.gscale * acc.z, a.gscale * acc.w);
        if (a.add) {
            const float4 p = *dst;
            o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w;
        }
        *dst = o;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.tick_a) *a.tick_a += 1;
        if (a.tick_b) *a.tick_b += 1;
    }
}

static size_t afft_lds_bytes(int H, int Q, int n_head, bool step) {
    return ((size_t)Q * H + (step ? (size_t)Q * n_head : 0)) * sizeof(float);
}

static int afft_common_ok(const r3d_afft_head_args& a) {
    if (!(a.fused && a.w_head && a.b_head && a.pooled && a.out)) return 0;
    if (!(a.B > 0 && a.S > 0 && a.K > 0 && a.n_head == a.K + 1 && a.ld_fused >= a.H && a.ld_out >= a.n_head)) return 0;
    if ((int64_t)a.B * a.S > (1ll << 30) / 4) return 0;            // unit and row indices stay in int
    return 1;
}

}  // namespace r3d

using namespace r3d;

/* 1: the pooled-head chain takes hidden H, Q queries and n_head = K + 1 head outputs (host-only): H % 4 == 0, H <= 1024,
 * Q <= 64, n_head <= 1024 and Q * (H + n_head) floats within 152 KiB of LDS. */
R3D_EXPORT int r3d_afft_head_supported(int H, int Q, int n_head) {
    if (H <= 0 || H % 4 || H > kAfftMaxH || Q <= 0 || Q > kAfftMaxQ || n_head < 2 || n_head > kAfftMaxHeads) return 0;
    return afft_lds_bytes(H, Q, n_head, true) <= kAfftMaxLds ? 1 : 0;
}

R3D_EXPORT int r3d_afft_head_fwd(const r3d_afft_head_args* p, void* stream) {
    R3D_REQUIRE(p);
    const r3d_afft_head_args& a = *p;
    R3D_REQUIRE(afft_common_ok(a));
    if (!r3d_afft_head_supported(a.H, a.Q, a.n_head)) return R3D_EINVAL;
    if (!r3d_aligned16(a.fused) || !r3d_aligned16(a.pooled) || a.ld_fused % 4) return R3D_EALIGN;
    const size_t lds = afft_lds_bytes(a.H, a.Q, a.n_head, false);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)afft_head_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(afft_head_fwd_kernel, dim3(a.B), dim3(kAfftThreads), lds, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

/* ws: r3d_losses_ws_floats(B, S, Q) floats; every unit the reduction reads is written here (see the head of this file). */
R3D_EXPORT int r3d_afft_head_step(const r3d_afft_head_args* p, float* ws, void* stream) {
    R3D_REQUIRE(p && ws);
    const r3d_afft_head_args& a = *p;
    R3D_REQUIRE(afft_common_ok(a));
    R3D_REQUIRE(a.past_label && a.target && a.target_dur && a.d_out && a.d_fused);
    R3D_REQUIRE(a.ld_dout >= a.n_head && a.ld_dfused >= a.H && (a.add == 0 || a.add == 1));
    if (!r3d_afft_head_supported(a.H, a.Q, a.n_head)) return R3D_EINVAL;
    if (!r3d_aligned16(a.fused) || !r3d_aligned16(a.pooled) || !r3d_aligned16(a.w_head) || !r3d_aligned16(a.d_fused) ||
        !r3d_aligned16(ws) || a.ld_fused % 4 || a.ld_dfused % 4)
        return R3D_EALIGN;
    LossArgs la{nullptr, 0, a.out, a.ld_out, a.out + a.K, a.ld_out, a.past_label, a.target, a.target_dur, a.B, a.S, a.Q, a.K,
                a.pad_idx, a.exclude_idx, 0, a.dur_den, a.grad_scale, nullptr, 0, a.d_out, a.ld_dout, a.d_out + a.K,
                a.ld_dout, nullptr, nullptr, nullptr, nullptr};
    const size_t lds = afft_lds_bytes(a.H, a.Q, a.n_head, true);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)afft_head_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(afft_head_step_kernel, dim3(a.B), dim3(kAfftThreads), lds, (hipStream_t)stream, a, la, ws);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
