// Cross-clip attention (reference model/futr_unsupervised_temp3.py:99-102): nn.MultiheadAttention(batch_first=True) called on
// the activations AFTER 'b t c -> t b c', so its batch is the S frame indices and its sequence is the B clips of the batch.
// For each frame t and head h the B rows { b S + t } attend to one another, without mask or dropout:
//   o[b S + t, h] = sum_c softmax_c(q[b S + t, h] . k[c S + t, h] / sqrt(dh)) v[c S + t, h].
//
// The rows are read in place from the [B S, 3 H] in-projection output (row stride ld): a workgroup owns FT consecutive frames
// and HG consecutive heads, and stages, per clip and part (q, k, v; d_o in the backward), FT runs of HG dh contiguous floats
// -- with all heads in the group, whole rows -- with 16-byte loads where the addresses allow it.  No transposed copy of the
// activations exists.  The B x B scores of a (frame, head) unit live in LDS only; the backward recomputes the probabilities
// from q and k (nothing but o crosses from the forward), so the op keeps no S heads B^2 tensor.
//
// Every sum runs in a fixed order inside one thread (no atomics, no cross-thread float reduction): the same call gives the
// same bits.  Each output element is written by exactly one thread, once: d_qkv is written in full, not accumulated.
#include "common.h"

namespace r3d {

constexpr int XC_MAX_B = 64, XC_MAX_DH = 128, XC_MAX_FT = 4, XC_THREADS = 256;
constexpr int XC_LDS_TARGET = 48 * 1024, XC_LDS_LIMIT = 160 * 1024;

struct XclipArgs {
    const float* qkv; int ld;
    float* o; int ldo;
    const float* d_o; int lddo;
    float* dqkv; int lddq;
    int B, S, H, heads, dh, FT, HG;
    float scale;
};

// LDS layout, in floats: NP parts (q, k, v[, d_o]) of B clips, clip stride CS (odd: the clips of one column fall in
// different banks), element (b, f, c) at b CS + f CW + c with CW = HG dh; then FT HG score matrices of B rows, row stride BP
// (odd); then, backward only, FT HG B row terms.
struct XclipLds {
    int CW, CS, PS, BP, US, off_s, off_d, total;
};
__host__ __device__ inline XclipLds xclip_lds(int B, int dh, int FT, int HG, int NP) {
    XclipLds l;
    l.CW = HG * dh;
    l.CS = (FT * l.CW) | 1;
    l.PS = B * l.CS;
    l.BP = B | 1;
    l.US = B * l.BP;
    l.off_s = NP * l.PS;
    l.off_d = l.off_s + FT * HG * l.US;
    l.total = l.off_d + (NP == 4 ? FT * HG * B : 0);
    return l;
}

static inline bool xclip_ok(int B, int dh) { return B >= 1 && B <= XC_MAX_B && dh >= 1 && dh <= XC_MAX_DH; }

// The frames and heads one workgroup owns: all heads and up to XC_MAX_FT frames while that stays within XC_LDS_TARGET (two
// workgroups per CU), else one frame and as many heads as fit; a single (frame, head) unit always fits the 160 KiB of a CU.
static void xclip_plan(int B, int S, int heads, int dh, int NP, int* FT, int* HG) {
    const auto bytes = [&](int ft, int hg) { return (size_t)xclip_lds(B, dh, ft, hg, NP).total * sizeof(float); };
    int ft = 1, hg = heads;
    while (hg > 1 && bytes(1, hg) > (size_t)XC_LDS_TARGET) --hg;
    if (hg == heads)
        while (ft < XC_MAX_FT && ft < S && bytes(ft + 1, hg) <= (size_t)XC_LDS_TARGET) ++ft;
    *FT = ft;
    *HG = hg;
}

// ---------------------------------------------------------------------------------------------------------------------
// staging: part rows [B, FT, CWa] from src (row stride ld, first column col0) into LDS
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void xclip_stage(float* __restrict__ dst, const XclipLds& l, const float* __restrict__ src, int ld,
                                            int col0, int B, int S, int t0, int FTa, int CWa) {
    const int tid = threadIdx.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) && (ld & 3) == 0 && (col0 & 3) == 0 && (CWa & 3) == 0;
    if (vec) {
        const int c4n = CWa >> 2, n = B * FTa * c4n;
        for (int w = tid; w < n; w += XC_THREADS) {
            const int c4 = w % c4n, r = w / c4n, f = r % FTa, b = r / FTa;
            const float4 v = *reinterpret_cast<const float4*>(src + ((size_t)b * S + t0 + f) * ld + col0 + 4 * c4);
            float* d = dst + b * l.CS + f * l.CW + 4 * c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        const int n = B * FTa * CWa;
        for (int w = tid; w < n; w += XC_THREADS) {
            const int c = w % CWa, r = w / CWa, f = r % FTa, b = r / FTa;
            dst[b * l.CS + f * l.CW + c] = src[((size_t)b * S + t0 + f) * ld + col0 + c];
        }
    }
}

// sc[u][i][j] = softmax_j(scale q_i . k_j) for every unit u = f HGa + hl of the workgroup
__device__ __forceinline__ void xclip_probs(const float* __restrict__ q, const float* __restrict__ k, float* __restrict__ sc,
                                            const XclipLds& l, int B, int dh, int FTa, int HGa, float scale) {
    const int tid = threadIdx.x, BB = B * B, n = FTa * HGa * BB;
    for (int w = tid; w < n; w += XC_THREADS) {
        const int j = w % B, i = (w / B) % B, u = w / BB, hl = u % HGa, f = u / HGa;
        const float* qp = q + i * l.CS + f * l.CW + hl * dh;
        const float* kp = k + j * l.CS + f * l.CW + hl * dh;
        float s = 0.f;
        for (int d = 0; d < dh; ++d) s = fmaf(qp[d], kp[d], s);
        sc[u * l.US + i * l.BP + j] = s * scale;
    }
    __syncthreads();
    const int rows = FTa * HGa * B;
    for (int w = tid; w < rows; w += XC_THREADS) {
        float* row = sc + (w / B) * l.US + (w % B) * l.BP;
        float mx = row[0];
        for (int j = 1; j < B; ++j) mx = fmaxf(mx, row[j]);
        float sum = 0.f;
        for (int j = 0; j < B; ++j) {
            const float e = expf(row[j] - mx);
            row[j] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int j = 0; j < B; ++j) row[j] *= inv;
    }
    __syncthreads();
}

// out[(r S + t0 + f) ldo + col0 + hl dh + d] = alpha sum_x coef(u, r, x) src[x, f, hl dh + d]; coef(u, r, x) = sc[u][r][x]
// (TRANS = false) or sc[u][x][r] (TRANS = true).  Work items run (f, r, hl, d): a row's columns are contiguous in memory.
template <bool TRANS>
__device__ __forceinline__ void xclip_apply(const float* __restrict__ sc, const float* __restrict__ src, const XclipLds& l,
                                            float* __restrict__ out, int ldo, int col0, int B, int S, int dh, int t0, int FTa,
                                            int HGa, float alpha) {
    const int tid = threadIdx.x, CWa = HGa * dh, n = FTa * B * CWa;
    for (int w = tid; w < n; w += XC_THREADS) {
        const int c = w % CWa, r = (w / CWa) % B, f = w / (CWa * B), hl = c / dh, u = f * HGa + hl;
        const float* sp = sc + u * l.US + (TRANS ? r : r * l.BP);
        const int ss = TRANS ? l.BP : 1;
        const float* vp = src + f * l.CW + c;
        float acc = 0.f;
        for (int x = 0; x < B; ++x) acc = fmaf(sp[x * ss], vp[x * l.CS], acc);
        out[((size_t)r * S + t0 + f) * ldo + col0 + c] = acc * alpha;
    }
}

__global__ __launch_bounds__(XC_THREADS) void xclip_fwd_kernel(const XclipArgs a) {
    extern __shared__ __align__(16) float xc_lds[];
    const XclipLds l = xclip_lds(a.B, a.dh, a.FT, a.HG, 3);
    const int t0 = blockIdx.x * a.FT, h0 = blockIdx.y * a.HG;
    const int FTa = min(a.FT, a.S - t0), HGa = min(a.HG, a.heads - h0), CWa = HGa * a.dh, col0 = h0 * a.dh;
    float *q = xc_lds, *k = q + l.PS, *v = k + l.PS, *sc = xc_lds + l.off_s;
    xclip_stage(q, l, a.qkv, a.ld, col0, a.B, a.S, t0, FTa, CWa);
    xclip_stage(k, l, a.qkv, a.ld, a.H + col0, a.B, a.S, t0, FTa, CWa);
    xclip_stage(v, l, a.qkv, a.ld, 2 * a.H + col0, a.B, a.S, t0, FTa, CWa);
    __syncthreads();
    xclip_probs(q, k, sc, l, a.B, a.dh, FTa, HGa, a.scale);
    xclip_apply<false>(sc, v, l, a.o, a.ldo, col0, a.B, a.S, a.dh, t0, FTa, HGa, 1.0f);
}

// With P the probabilities, dP_ij = d_o_i . v_j and delta_i = sum_j P_ij dP_ij:
//   dv_j = sum_i P_ij d_o_i,  dS_ij = P_ij (dP_ij - delta_i),  dq_i = scale sum_j dS_ij k_j,  dk_j = scale sum_i dS_ij q_i.
__global__ __launch_bounds__(XC_THREADS) void xclip_bwd_kernel(const XclipArgs a) {
    extern __shared__ __align__(16) float xc_lds[];
    const XclipLds l = xclip_lds(a.B, a.dh, a.FT, a.HG, 4);
    const int tid = threadIdx.x, B = a.B, dh = a.dh;
    const int t0 = blockIdx.x * a.FT, h0 = blockIdx.y * a.HG;
    const int FTa = min(a.FT, a.S - t0), HGa = min(a.HG, a.heads - h0), CWa = HGa * dh, col0 = h0 * dh;
    float *q = xc_lds, *k = q + l.PS, *v = k + l.PS, *g = v + l.PS, *sc = xc_lds + l.off_s, *delta = xc_lds + l.off_d;
    xclip_stage(q, l, a.qkv, a.ld, col0, B, a.S, t0, FTa, CWa);
    xclip_stage(k, l, a.qkv, a.ld, a.H + col0, B, a.S, t0, FTa, CWa);
    xclip_stage(v, l, a.qkv, a.ld, 2 * a.H + col0, B, a.S, t0, FTa, CWa);
    xclip_stage(g, l, a.d_o, a.lddo, col0, B, a.S, t0, FTa, CWa);
    __syncthreads();
    xclip_probs(q, k, sc, l, B, dh, FTa, HGa, a.scale);
    const int rows = FTa * HGa * B;
    for (int w = tid; w < rows; w += XC_THREADS) {              // delta_i
        const int i = w % B, u = w / B, hl = u % HGa, f = u / HGa;
        const float* gp = g + i * l.CS + f * l.CW + hl * dh;
        const float* row = sc + u * l.US + i * l.BP;
        float acc = 0.f;
        for (int j = 0; j < B; ++j) {
            const float* vp = v + j * l.CS + f * l.CW + hl * dh;
            float dp = 0.f;
            for (int d = 0; d < dh; ++d) dp = fmaf(gp[d], vp[d], dp);
            acc = fmaf(row[j], dp, acc);
        }
        delta[w] = acc;
    }
    xclip_apply<true>(sc, g, l, a.dqkv, a.lddq, 2 * a.H + col0, B, a.S, dh, t0, FTa, HGa, 1.0f);         // dv
    __syncthreads();
    const int BB = B * B, n = FTa * HGa * BB;
    for (int w = tid; w < n; w += XC_THREADS) {                 // dS over P, in place
        const int j = w % B, i = (w / B) % B, u = w / BB, hl = u % HGa, f = u / HGa;
        const float* gp = g + i * l.CS + f * l.CW + hl * dh;
        const float* vp = v + j * l.CS + f * l.CW + hl * dh;
        float dp = 0.f;
        for (int d = 0; d < dh; ++d) dp = fmaf(gp[d], vp[d], dp);
        float* p = sc + u * l.US + i * l.BP + j;
        *p = *p * (dp - delta[u * B + i]);
    }
    __syncthreads();
    xclip_apply<false>(sc, k, l, a.dqkv, a.lddq, col0, B, a.S, dh, t0, FTa, HGa, a.scale);              // dq
    xclip_apply<true>(sc, q, l, a.dqkv, a.lddq, a.H + col0, B, a.S, dh, t0, FTa, HGa, a.scale);         // dk
}

static int xclip_launch(XclipArgs a, bool bwd, void* stream) {
    if (!a.qkv || a.S < 1 || a.heads < 1 || a.dh < 1 || !xclip_ok(a.B, a.dh)) return R3D_EINVAL;
    a.H = a.heads * a.dh;
    if (a.ld < 3 * a.H || (int64_t)a.B * a.S * 3 * a.H >= (int64_t)1 << 31) return R3D_EINVAL;
    if (!bwd && (!a.o || a.ldo < a.H)) return R3D_EINVAL;
    if (bwd && (!a.d_o || !a.dqkv || a.lddo < a.H || a.lddq < 3 * a.H)) return R3D_EINVAL;
    const int NP = bwd ? 4 : 3;
    xclip_plan(a.B, a.S, a.heads, a.dh, NP, &a.FT, &a.HG);
    const size_t lds = (size_t)xclip_lds(a.B, a.dh, a.FT, a.HG, NP).total * sizeof(float);
    if (lds > (size_t)XC_LDS_LIMIT) return R3D_EINVAL;
    if (r3d_cdiv(a.heads, a.HG) > 65535) return R3D_EINVAL;
    a.scale = 1.0f / sqrtf((float)a.dh);
    const void* fn = bwd ? (const void*)xclip_bwd_kernel : (const void*)xclip_fwd_kernel;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid(r3d_cdiv(a.S, a.FT), r3d_cdiv(a.heads, a.HG));
    if (bwd)
        hipLaunchKernelGGL(xclip_bwd_kernel, grid, dim3(XC_THREADS), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(xclip_fwd_kernel, grid, dim3(XC_THREADS), lds, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_xclip_supported(int B, int dh) { return xclip_ok(B, dh) ? 1 : 0; }

R3D_EXPORT int r3d_xclip_frame_run(int B, int S, int heads, int dh, int bwd) {
    if (!xclip_ok(B, dh) || S < 1 || heads < 1) return 0;
    int ft, hg;
    xclip_plan(B, S, heads, dh, bwd ? 4 : 3, &ft, &hg);
    return ft;
}

R3D_EXPORT int r3d_xclip_fwd(const float* qkv, int ld, float* o, int ldo, int B, int S, int heads, int dh, void* stream) {
    XclipArgs a{};
    a.qkv = qkv; a.ld = ld; a.o = o; a.ldo = ldo; a.B = B; a.S = S; a.heads = heads; a.dh = dh;
    return xclip_launch(a, false, stream);
}

R3D_EXPORT int r3d_xclip_bwd(const float* qkv, int ld, const float* d_o, int lddo, float* d_qkv, int lddq, int B, int S,
                             int heads, int dh, void* stream) {
    XclipArgs a{};
    a.qkv = qkv; a.ld = ld; a.d_o = d_o; a.lddo = lddo; a.dqkv = d_qkv; a.lddq = lddq; a.B = B; a.S = S; a.heads = heads;
    a.dh = dh;
    return xclip_launch(a, true, stream);
}
