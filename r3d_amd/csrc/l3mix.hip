// The loss mix of the L3 query loop (reference train/train_unsupervised.py:357-362).  With l2_correct[r] = [past_label[r] !=
// pad_idx and argmax(seg[r]) == past_label[r]] (torch's argmax: the first index of the maximum), l3_correct the focal launch's
// flags and N = B S rows,
//   m     = mean_r (l3_correct[r] && l2_correct[r] ? 1 : 5)                       (no gradient: it comes from arg-maxes)
//   total = (1 - 1/m) ((1 - wf) L_3 + wf L_c) + (1/m) (L_act + L_dur + L_seg)
// Two launches.  rows: one wave per row forms l2_correct and each workgroup leaves the count of its rows with both flags set
// (an integer, so the sum below has one value whatever the order).  apply: every workgroup sums those counts in a fixed order,
// forms m and c = 1/m, and scales its share of d_seg and d_actdur by c in place; workgroup 0 writes out[5] = (m, a, b, c,
// total) with a = (1 - 1/m)(1 - wf), b = (1 - 1/m) wf -- the device scalars the focal and cluster backward launches take as
// d_loss.  wf is a device scalar.  No atomics, no read-back.
#include "common.h"

namespace r3d {

constexpr int MIX_ROWS = 4;            // rows (waves) per workgroup of the rows launch

struct MixArgs {
    const float* seg; int ld_seg;
    const int64_t* label;
    const uint8_t* l3_flags;
    int N, Kseg, pad_idx;
    uint8_t* l2_flags;
    int* part; int nparts;
    const float* l3; const float* lc; const float* loss3; const float* wf;
    float* d_seg; int ld_dseg;
    float* d_actdur; int rows_ad, cols_ad, ld_dad;
    float* out;
};

__global__ __launch_bounds__(256) void l3mix_rows_kernel(const MixArgs a) {
    __shared__ int both[MIX_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, row = blockIdx.x * MIX_ROWS + w;
    int hit = 0;
    if (row < a.N) {
        const float* xp = a.seg + (size_t)row * a.ld_seg;
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int c = lane; c < a.Kseg; c += 64) {
            const float v = xp[c];
            if (v > best || arg == 0x7fffffff) {
                best = v;
                arg = c;
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                      // the largest value, the lowest index among equals
            const float ov = __shfl_xor(best, o);
            const int oa = __shfl_xor(arg, o);
            if (oa != 0x7fffffff && (arg == 0x7fffffff || ov > best || (ov == best && oa < arg))) {
                best = ov;
                arg = oa;
            }
        }
        const int64_t g = a.label[row];
        const int l2 = g != (int64_t)a.pad_idx && (int64_t)arg == g ? 1 : 0;
        hit = l2 && a.l3_flags[row] ? 1 : 0;
        if (lane == 0 && a.l2_flags) a.l2_flags[row] = (uint8_t)l2;
    }
    if (lane == 0) both[w] = hit;
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = (both[0] + both[1]) + (both[2] + both[3]);
}

__global__ __launch_bounds__(256) void l3mix_apply_kernel(const MixArgs a) {
    __shared__ int red[256];
    const int tid = threadIdx.x;
    int cnt = 0;
    for (int i = tid; i < a.nparts; i += 256) cnt += a.part[i];
    red[tid] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    cnt = red[0];
    // the mean of N values 1 or 5 as torch forms it: their float sum (exact below 2^24) over N
    const double sum = 5.0 * (double)a.N - 4.0 * (double)cnt;
    const float m = sum < 16777216.0 ? (float)sum / (float)a.N : (float)(sum / (double)a.N);
    const float c = 1.0f / m, r = 1.0f - c;
    if (blockIdx.x == 0 && tid == 0) {
        const float wf = a.wf[0];
        a.out[0] = m;
        a.out[1] = r * (1.0f - wf);
        a.out[2] = r * wf;
        a.out[3] = c;
        a.out[4] = r * ((1.0f - wf) * a.l3[0] + wf * a.lc[0]) + c * ((a.loss3[1] + a.loss3[2]) + a.loss3[0]);
    }
    const int64_t gstride = (int64_t)gridDim.x * 256, g0 = (int64_t)blockIdx.x * 256 + tid;
    if (a.d_seg) {
        const int64_t n = (int64_t)a.N * a.Kseg;
        for (int64_t i = g0; i < n; i += gstride) {
            float* p = a.d_seg + (i / a.Kseg) * a.ld_dseg + (i % a.Kseg);
            *p *= c;
        }
    }
    if (a.d_actdur) {
        const int64_t n = (int64_t)a.rows_ad * a.cols_ad;
        for (int64_t i = g0; i < n; i += gstride) {
            float* p = a.d_actdur + (i / a.cols_ad) * a.ld_dad + (i % a.cols_ad);
            *p *= c;
        }
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int64_t r3d_l3mix_ws_ints(int N) { return N >= 1 ? (int64_t)r3d_cdiv(N, MIX_ROWS) : 0; }

R3D_EXPORT int r3d_l3mix(const float* seg, int ld_seg, const int64_t* past_label, const uint8_t* l3_flags, int N, int Kseg,
                         int pad_idx, const float* l3, const float* lc, const float* loss3, const float* wf, float* d_seg,
                         int ld_dseg, float* d_actdur, int rows_ad, int cols_ad, int ld_dad, uint8_t* l2_flags, int* ws,
                         float* out, void* stream) {
    if (!seg || !past_label || !l3_flags || !l3 || !lc || !loss3 || !wf || !ws || !out) return R3D_EINVAL;
    if (N < 1 || N > (1 << 30) || Kseg < 1 || ld_seg < Kseg) return R3D_EINVAL;
    if (d_seg && ld_dseg < Kseg) return R3D_EINVAL;
    if (d_actdur && (rows_ad < 1 || cols_ad < 1 || ld_dad < cols_ad)) return R3D_EINVAL;
    MixArgs a{};
    a.seg = seg; a.ld_seg = ld_seg; a.label = past_label; a.l3_flags = l3_flags; a.N = N; a.Kseg = Kseg; a.pad_idx = pad_idx;
    a.l2_flags = l2_flags; a.part = ws; a.nparts = r3d_cdiv(N, MIX_ROWS); a.l3 = l3; a.lc = lc; a.loss3 = loss3; a.wf = wf;
    a.d_seg = d_seg; a.ld_dseg = ld_dseg; a.d_actdur = d_actdur; a.rows_ad = rows_ad; a.cols_ad = cols_ad; a.ld_dad = ld_dad;
    a.out = out;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(l3mix_rows_kernel, dim3(a.nparts), dim3(256), 0, s, a);
    R3D_LAUNCH_CHECK();
    int64_t work = d_seg ? (int64_t)N * Kseg : 0;
    if (d_actdur && (int64_t)rows_ad * cols_ad > work) work = (int64_t)rows_ad * cols_ad;
    int64_t blocks = (work + 1023) / 1024;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(l3mix_apply_kernel, dim3((int)blocks), dim3(256), 0, s, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
