// Dilated causal Conv1d (kernel 3) with weight normalisation, for the TCN baseline (reference model/tcn.py).
// See include/r3d_hip.h "temporal convolution" for the contract.
//
// Activations are [B*S, C] row-major (a clip's frames consecutive).  Tap j of the [C_out, C_in, 3] weight reads frame
// t - (2 - j) d of the SAME clip, zeros before frame 0.  All three products are fp32-MFMA tile GEMMs
// (v_mfma_f32_32x32x2_f32, exact fp32 fma chains) whose operand LOADER applies the frame shift and the clip mask while
// it stages the tile into LDS -- there is no im2col copy of an activation anywhere:
//   forward        P[r, o]     = sum_{j,c} X[r - (2-j)d, c] v[o, c, j]              (rows with t < (2-j)d are zero)
//   input gradient dX[r, c]    = sum_{j,o} s_o dZ[r + (2-j)d, o] v[o, c, j]         (rows with t + (2-j)d >= S are zero)
//   weight gradient G[o, c, j] = sum_r dZ[r, o] X[r - (2-j)d, c]
// The mask is computed from t = r % S, so a shifted row index is never dereferenced across a clip boundary (and never
// outside the tensor: a masked load reads row 0 of the tensor and its value is discarded).
// Weight normalisation never materialises g v / |v|: the forward runs on weight_v and applies s_o = g_o / |v_o| in its
// epilogue; the weight-gradient epilogue turns the raw G into dv = s (G - <G_o, v_o> v / |v_o|^2), where <G_o, v_o> =
// sum_r dZ[r, o] P[r, o] comes from tconv_bwd_prep (column sums in a fixed order: row chunks, then chunk by chunk).
// No atomics: every reduction has one order, so a step is bitwise reproducible.
//
// Tile scheme: 64 x 64 output per workgroup of 4 waves (2 x 2, one 32x32 MFMA tile each), both operands K-contiguous in
// LDS (row stride K + 4 floats: a ds_read_b128 of 4 consecutive k feeds four MFMAs; the padding is not a measured claim about bank conflicts), global loads of the
// next step are issued into registers before the MFMAs of the current one.  The operand whose global layout interleaves
// the taps (the weight: (c, j) pairs are contiguous) is read with 16-byte loads and scattered into LDS tap-major.
#include "common.h"
#include "../../include/r3d_hip.h"

namespace r3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TC_T = 64;                 // output tile edge
constexpr int TC_KC = 32;                // reduction channels (rows for the weight gradient) per tap and step
constexpr int TC_LS = 3 * TC_KC + 4;     // LDS row stride of the row products (3 taps x 32 channels)
constexpr int TC_LW = TC_KC + 4;         // LDS row stride of the weight gradient
constexpr int TC_RC = 256;               // rows per chunk of the column reductions

struct TconvRows {
    const float* A; int lda;             // fwd: X [M, Kc]; dx: dZ [M, Kc]
    const float* V;                      // weight_v [C_out, C_in, 3]
    const float* kscale;                 // dx: s [Kc] scales A's columns
    int M, S, N, Kc, dil, Cin;
    const float* s; const float* bias;   // fwd epilogue
    float* P; int ldp; float* Y; int ldy;
    const uint8_t* drop; float drop_scale;
    const float* res; int ldres; float* out; int ldout;
    const float* gate; int ldgate;       // dx epilogue
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// MODE 0: forward, MODE 1: input gradient
template <int MODE>
__global__ __launch_bounds__(256) void tconv_rows_kernel(TconvRows a) {
    __shared__ float As[TC_T * TC_LS];
    __shared__ float Bs[TC_T * TC_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * TC_T, n0 = blockIdx.x * TC_T;
    const size_t wrow = (size_t)3 * a.Cin;

    // per-thread constants of the 6 A pieces: tap j = p >> 1, row = rem >> 3, channel quad = rem & 7
    const float* asrc[6];
    bool aok[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const int j = p >> 1, rem = tid + (p & 1) * 256;
        const int m = m0 + (rem >> 3);
        const int shift = (2 - j) * a.dil;
        const int t = m % a.S;
        const bool ok = m < a.M && (MODE == 0 ? t >= shift : t + shift < a.S);
        const int src = ok ? (MODE == 0 ? m - shift : m + shift) : 0;
        aok[p] = ok;
        asrc[p] = a.A + (size_t)src * a.lda + ((rem & 7) << 2);
    }
    // the 6 B pieces
    const float* bsrc[6];
    bool bok[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const int f = tid + p * 256;
        if (MODE == 0) {                                 // 64 weight rows x 24 float4 of (c, j) pairs
            const int n = n0 + f / 24, q = f % 24;
            bok[p] = n < a.N;
            bsrc[p] = a.V + (size_t)(bok[p] ? n : 0) * wrow + 4 * q;
        } else {                                         // 32 weight rows (o) x 48 float4 of (c, j) pairs
            const int q = f % 48;
            bok[p] = n0 * 3 + 4 * q + 3 < 3 * a.N;
            bsrc[p] = a.V + (size_t)(f / 48) * wrow + (bok[p] ? n0 * 3 + 4 * q : 0);
        }
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    float4 ra[6], rb[6];
    auto load = [&](int kc0) {
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            float4 v = ld4(asrc[p] + kc0);
            if (MODE == 1) {
                const float4 s4 = ld4(a.kscale + kc0 + (((tid + (p & 1) * 256) & 7) << 2));
                v.x *= s4.x; v.y *= s4.y; v.z *= s4.z; v.w *= s4.w;
            }
            ra[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p)
            rb[p] = ld4(MODE == 0 ? bsrc[p] + (size_t)kc0 * 3 : bsrc[p] + (size_t)kc0 * wrow);
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const int j = p >> 1, rem = tid + (p & 1) * 256;
            float4 v = ra[p];
            if (!aok[p]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(As + (rem >> 3) * TC_LS + j * TC_KC + ((rem & 7) << 2)) = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const int f = tid + p * 256;
            const float e[4] = {rb[p].x, rb[p].y, rb[p].z, rb[p].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = bok[p] ? e[i] : 0.f;
                if (MODE == 0) {
                    const int idx = 4 * (f % 24) + i;                    // = c_local * 3 + j
                    Bs[(f / 24) * TC_LS + (idx % 3) * TC_KC + idx / 3] = x;
                } else {
                    const int idx = 4 * (f % 48) + i;                    // = c_local * 3 + j, row f / 48 = o_local
                    Bs[(idx / 3) * TC_LS + (idx % 3) * TC_KC + f / 48] = x;
                }
            }
        }
    };

    const int nk = a.Kc / TC_KC;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        store();
        __syncthreads();
        if (kt + 1 < nk) load((kt + 1) * TC_KC);
#pragma unroll
        for (int g = 0; g < 3 * TC_KC / 8; ++g) {
            const int kb = g * 8 + 4 * lhi;
            const float4 a4 = ld4(As + (wm * 32 + l31) * TC_LS + kb);
            const float4 b4 = ld4(Bs + (wn * 32 + l31) * TC_LS + kb);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
        }
    }

    const int n = n0 + wn * 32 + l31;
    if (n >= a.N) return;
    float sn = 0.f, bn = 0.f;
    if (MODE == 0) { sn = a.s[n]; bn = a.bias[n]; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (m >= a.M) continue;
        float v = acc[r];
        if (MODE == 0) {
            if (a.P) a.P[(size_t)m * a.ldp + n] = v;
            v = fmaxf(sn * v + bn, 0.f);
            if (a.drop) v *= a.drop_scale * (float)a.drop[(size_t)m * a.N + n];
            a.Y[(size_t)m * a.ldy + n] = v;
            if (a.out) a.out[(size_t)m * a.ldout + n] = fmaxf(v + a.res[(size_t)m * a.ldres + n], 0.f);
        } else {
            if (a.res) v += a.res[(size_t)m * a.ldres + n];
            if (a.gate) v = a.gate[(size_t)m * a.ldgate + n] > 0.f ? v : 0.f;
            a.out[(size_t)m * a.ldout + n] = v;
        }
    }
}

struct TconvWgrad {
    const float* dZ; int lddz; const float* X; int ldx;
    const float* V; const float* s; const float* coef;
    float* G;
    int M, S, Cin, Cout, dil;
    int splits, rows_per_split;          // splits > 1: blockIdx.z owns a row range and writes its raw tile to part[z]
    float* part;
};

// G tile of 64 o x 64 c x 3 taps; reduction over the rows r, 32 per step.  dZ and X arrive row-major (o / c contiguous)
// and are scattered transposed into LDS so that the MFMA operands are K-contiguous.
__global__ __launch_bounds__(256) void tconv_wgrad_kernel(TconvWgrad a) {
    __shared__ float As[TC_T * TC_LW];
    __shared__ float Bs[3 * TC_T * TC_LW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int o0 = blockIdx.y * TC_T, c0 = blockIdx.x * TC_T;
    const int rl = tid >> 4, q4 = (tid & 15) << 2;        // piece p covers local row rl + 16 * (p & 1)
    const bool aco = o0 + q4 < a.Cout, bco = c0 + q4 < a.Cin;
    const int acol = aco ? o0 + q4 : 0, bcol = bco ? c0 + q4 : 0;

    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    float4 ra[2], rb[6];
    bool aok[2], bok[6];
    auto load = [&](int r0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = r0 + rl + 16 * p;
            aok[p] = r < a.M && aco;
            ra[p] = ld4(a.dZ + (size_t)(r < a.M ? r : 0) * a.lddz + acol);
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const int j = p >> 1, r = r0 + rl + 16 * (p & 1);
            const int shift = (2 - j) * a.dil;
            const bool ok = r < a.M && (r % a.S) >= shift;
            bok[p] = ok && bco;
            rb[p] = ld4(a.X + (size_t)(ok ? r - shift : 0) * a.ldx + bcol);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float e[4] = {ra[p].x, ra[p].y, ra[p].z, ra[p].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) As[(q4 + i) * TC_LW + rl + 16 * p] = aok[p] ? e[i] : 0.f;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const float e[4] = {rb[p].x, rb[p].y, rb[p].z, rb[p].w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                Bs[((p >> 1) * TC_T + q4 + i) * TC_LW + rl + 16 * (p & 1)] = bok[p] ? e[i] : 0.f;
        }
    };

    const int rbeg = blockIdx.z * a.rows_per_split;                     // (a multiple of TC_KC)
    const int rend = min(a.M, rbeg + a.rows_per_split);
    const int nk = (rend - rbeg + TC_KC - 1) / TC_KC;
    a.M = rend;                                                         // rows beyond the split's range load as zeros
    load(rbeg);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        store();
        __syncthreads();
        if (kt + 1 < nk) load(rbeg + (kt + 1) * TC_KC);
#pragma unroll
        for (int g = 0; g < TC_KC / 8; ++g) {
            const int kb = g * 8 + 4 * lhi;
            const float4 a4 = ld4(As + (wm * 32 + l31) * TC_LW + kb);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 b4 = ld4(Bs + (j * TC_T + wn * 32 + l31) * TC_LW + kb);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc[j], 0, 0, 0);
            }
        }
    }

    const int c = c0 + wn * 32 + l31;
    if (c >= a.Cin) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (o >= a.Cout) continue;
        const size_t base = ((size_t)o * a.Cin + c) * 3;
        if (a.splits > 1) {
            float* dst = a.part + (size_t)blockIdx.z * 3 * a.Cin * a.Cout + base;
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[j] = acc[j][r];
            continue;
        }
        const float so = a.s ? a.s[o] : 1.f, co = a.coef ? a.coef[o] : 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) a.G[base + j] = so * (acc[j][r] - co * (a.coef ? a.V[base + j] : 0.f));
    }
}

// The split form's second half: G = sum of the partial tiles, split by split, then the weight-norm epilogue.
__global__ __launch_bounds__(256) void tconv_wgrad_fin_kernel(TconvWgrad a) {
    const size_t n = (size_t)3 * a.Cin * a.Cout;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 g = ld4(a.part + i);
    for (int z = 1; z < a.splits; ++z) {
        const float4 t = ld4(a.part + (size_t)z * n + i);
        g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
    }
    float e[4] = {g.x, g.y, g.z, g.w};
    const size_t row = (size_t)3 * a.Cin;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = (int)((i + k) / row);
        const float so = a.s ? a.s[o] : 1.f;
        e[k] = so * (e[k] - (a.coef ? a.coef[o] * a.V[i + k] : 0.f));
    }
    *reinterpret_cast<float4*>(a.G + i) = make_float4(e[0], e[1], e[2], e[3]);
}

// Sums 256 per-thread values over the workgroup in a fixed order; every thread gets the result.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// s_o = g_o / |v_o|, inv_o = 1 / |v_o|: one workgroup per output channel.
__global__ __launch_bounds__(256) void tconv_wnorm_kernel(const float* __restrict__ v, const float* __restrict__ g, int len,
                                                         float* __restrict__ s, float* __restrict__ inv) {
    __shared__ float red[4];
    const float* row = v + (size_t)blockIdx.x * len;
    float acc = 0.f;
    for (int i = threadIdx.x * 4; i < len; i += 1024) {
        const float4 x = ld4(row + i);
        acc += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
    }
    const float tot = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        const float r = 1.0f / sqrtf(tot);
        inv[blockIdx.x] = r;
        s[blockIdx.x] = g[blockIdx.x] * r;
    }
}

// dZ = (y > 0) ? scale * dY : 0 (the adjoint of dropout(relu(.)): y > 0 iff the pre-activation was positive and the
// element was kept), plus the chunk's column sums of dZ and dZ * P.  part: [chunks][2][C].
__global__ __launch_bounds__(256) void tconv_bwd_prep_kernel(const float* __restrict__ dY, int lddy, const float* __restrict__ Y,
                                                            int ldy, const float* __restrict__ P, int ldp, float scale,
                                                            float* __restrict__ dZ, int lddz, int M, int C,
                                                            float* __restrict__ part) {
    __shared__ float red[2][4][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const int r0 = blockIdx.y * TC_RC;
    const int r1 = min(M, r0 + TC_RC);
    float sb = 0.f, sd = 0.f;
    if (c < C) {
        for (int r = r0 + ry; r < r1; r += 4) {
            const float y = Y[(size_t)r * ldy + c];
            const float d = y > 0.f ? scale * dY[(size_t)r * lddy + c] : 0.f;
            dZ[(size_t)r * lddz + c] = d;
            sb += d;
            sd += d * P[(size_t)r * ldp + c];
        }
    }
    red[0][ry][cx] = sb;
    red[1][ry][cx] = sd;
    __syncthreads();
    if (ry == 0 && c < C) {
        part[((size_t)blockIdx.y * 2 + 0) * C + c] = (red[0][0][cx] + red[0][1][cx]) + (red[0][2][cx] + red[0][3][cx]);
        part[((size_t)blockIdx.y * 2 + 1) * C + c] = (red[1][0][cx] + red[1][1][cx]) + (red[1][2][cx] + red[1][3][cx]);
    }
}

// chunk by chunk: db_o = sum dZ, dot_o = <G_o, v_o>; dg_o = dot_o / |v_o|, coef_o = dot_o / |v_o|^2
__global__ void tconv_bwd_fin_kernel(const float* __restrict__ part, int chunks, int C, const float* __restrict__ inv,
                                     float* __restrict__ db, float* __restrict__ dg, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float sb = 0.f, sd = 0.f;
    for (int k = 0; k < chunks; ++k) {
        sb += part[((size_t)k * 2 + 0) * C + c];
        sd += part[((size_t)k * 2 + 1) * C + c];
    }
    const float r = inv[c];
    db[c] = sb;
    dg[c] = sd * r;
    coef[c] = sd * r * r;
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_tconv_supported(int rows, int S, int c_in, int c_out, int dilation) {
    if (rows < 1 || S < 1 || rows % S || c_in < TC_KC || c_out < TC_KC || c_in % TC_KC || c_out % TC_KC || dilation < 1) return 0;
    if (dilation > (1 << 20)) return 0;
    const int64_t big = (int64_t)1 << 31;
    if ((int64_t)rows * c_in >= big || (int64_t)rows * c_out >= big || (int64_t)3 * c_in * c_out >= big) return 0;
    if ((rows + TC_T - 1) / TC_T > 65535 || (rows + TC_RC - 1) / TC_RC > 65535) return 0;
    return 1;
}

R3D_EXPORT int64_t r3d_tconv_ws_floats(int rows, int c_out) {
    return (int64_t)((rows + TC_RC - 1) / TC_RC) * 2 * c_out;
}

// Row splits of the weight gradient: its output has few tiles (16 for 256 x 256) and a reduction as long as the batch, so
// the rows are cut into ranges of at least 128 until about two workgroups per CU exist.
static int tconv_wgrad_splits(int rows, int c_in, int c_out) {
    const int tiles = r3d_cdiv(c_in, TC_T) * r3d_cdiv(c_out, TC_T);
    const int nk = r3d_cdiv(rows, TC_KC);
    int s = r3d_cdiv(512, tiles);
    if (s > nk / 4) s = nk / 4;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

R3D_EXPORT int64_t r3d_tconv_wgrad_ws_floats(int rows, int c_in, int c_out) {
    if (rows < 1 || c_in < 1 || c_out < 1) return 0;
    const int s = tconv_wgrad_splits(rows, c_in, c_out);
    return s > 1 ? (int64_t)s * 3 * c_in * c_out : 0;
}

R3D_EXPORT int r3d_tconv_wnorm(const float* v, const float* g, int c_in, int c_out, float* s, float* inv_norm, void* stream) {
    R3D_REQUIRE(v && g && s && inv_norm && c_in >= 1 && c_out >= 1 && (3 * (int64_t)c_in) % 4 == 0);
    if (!r3d_aligned16(v)) return R3D_EALIGN;
    hipLaunchKernelGGL(tconv_wnorm_kernel, dim3(c_out), dim3(256), 0, (hipStream_t)stream, v, g, 3 * c_in, s, inv_norm);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_tconv_fwd(const float* x, int ldx, const float* v, const float* s, const float* bias, int rows, int S,
                             int c_in, int c_out, int dilation, float* p_out, int ldp, float* y, int ldy, const uint8_t* drop,
                             float drop_scale, const float* res, int ldres, float* out, int ldout, void* stream) {
    R3D_REQUIRE(x && v && s && bias && y && r3d_tconv_supported(rows, S, c_in, c_out, dilation));
    R3D_REQUIRE(ldx >= c_in && ldy >= c_out && (!p_out || ldp >= c_out) && (!out || (res && ldres >= c_out && ldout >= c_out)));
    if (!r3d_aligned16(x) || !r3d_aligned16(v) || ldx % 4) return R3D_EALIGN;
    TconvRows a = {};
    a.A = x; a.lda = ldx; a.V = v; a.M = rows; a.S = S; a.N = c_out; a.Kc = c_in; a.dil = dilation; a.Cin = c_in;
    a.s = s; a.bias = bias; a.P = p_out; a.ldp = ldp; a.Y = y; a.ldy = ldy; a.drop = drop; a.drop_scale = drop_scale;
    a.res = res; a.ldres = ldres; a.out = out; a.ldout = ldout;
    hipLaunchKernelGGL(tconv_rows_kernel<0>, dim3(r3d_cdiv(c_out, TC_T), r3d_cdiv(rows, TC_T)), dim3(256), 0,
                       (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_tconv_bwd_prep(const float* dy, int lddy, const float* y, int ldy, const float* p, int ldp, float drop_scale,
                                  const float* inv_norm, int rows, int c_out, float* dz, int lddz, float* d_bias, float* d_g,
                                  float* coef, float* ws, void* stream) {
    R3D_REQUIRE(dy && y && p && inv_norm && dz && d_bias && d_g && coef && ws && rows >= 1 && c_out >= 1);
    R3D_REQUIRE(lddy >= c_out && ldy >= c_out && ldp >= c_out && lddz >= c_out);
    const int chunks = r3d_cdiv(rows, TC_RC);
    R3D_REQUIRE(chunks <= 65535);
    hipLaunchKernelGGL(tconv_bwd_prep_kernel, dim3(r3d_cdiv(c_out, 64), chunks), dim3(256), 0, (hipStream_t)stream, dy, lddy, y,
                       ldy, p, ldp, drop_scale, dz, lddz, rows, c_out, ws);
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(tconv_bwd_fin_kernel, dim3(r3d_cdiv(c_out, 64)), dim3(64), 0, (hipStream_t)stream, ws, chunks, c_out,
                       inv_norm, d_bias, d_g, coef);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_tconv_dx(const float* dz, int lddz, const float* v, const float* s, int rows, int S, int c_in, int c_out,
                            int dilation, const float* res, int ldres, const float* gate, int ldgate, float* dx, int lddx,
                            void* stream) {
    R3D_REQUIRE(dz && v && s && dx && r3d_tconv_supported(rows, S, c_in, c_out, dilation));
    R3D_REQUIRE(lddz >= c_out && lddx >= c_in && (!res || ldres >= c_in) && (!gate || ldgate >= c_in));
    if (!r3d_aligned16(dz) || !r3d_aligned16(v) || !r3d_aligned16(s) || lddz % 4) return R3D_EALIGN;
    TconvRows a = {};
    a.A = dz; a.lda = lddz; a.V = v; a.kscale = s; a.M = rows; a.S = S; a.N = c_in; a.Kc = c_out; a.dil = dilation;
    a.Cin = c_in; a.res = res; a.ldres = ldres; a.gate = gate; a.ldgate = ldgate; a.out = dx; a.ldout = lddx;
    hipLaunchKernelGGL(tconv_rows_kernel<1>, dim3(r3d_cdiv(c_in, TC_T), r3d_cdiv(rows, TC_T)), dim3(256), 0,
                       (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_tconv_wgrad(const float* dz, int lddz, const float* x, int ldx, const float* v, const float* s,
                               const float* coef, int rows, int S, int c_in, int c_out, int dilation, float* d_v, float* ws,
                               void* stream) {
    R3D_REQUIRE(dz && x && d_v && r3d_tconv_supported(rows, S, c_in, c_out, dilation));
    R3D_REQUIRE(lddz >= c_out && ldx >= c_in && (!coef || (v && s)));
    if (!r3d_aligned16(dz) || !r3d_aligned16(x) || !r3d_aligned16(d_v) || lddz % 4 || ldx % 4) return R3D_EALIGN;
    TconvWgrad a = {};
    a.dZ = dz; a.lddz = lddz; a.X = x; a.ldx = ldx; a.V = v; a.s = s; a.coef = coef; a.G = d_v;
    a.M = rows; a.S = S; a.Cin = c_in; a.Cout = c_out; a.dil = dilation;
    a.splits = tconv_wgrad_splits(rows, c_in, c_out);
    a.rows_per_split = r3d_cdiv(r3d_cdiv(rows, a.splits), TC_KC) * TC_KC;
    a.splits = r3d_cdiv(rows, a.rows_per_split);                        // (no empty range)
    a.part = ws;
    if (a.splits > 1) {
        R3D_REQUIRE(ws);
        if (!r3d_aligned16(ws) || (coef && !r3d_aligned16(v))) return R3D_EALIGN;
    }
    hipLaunchKernelGGL(tconv_wgrad_kernel, dim3(r3d_cdiv(c_in, TC_T), r3d_cdiv(c_out, TC_T), a.splits), dim3(256), 0,
                       (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    if (a.splits > 1) {
        const size_t n4 = (size_t)3 * c_in * c_out / 4;
        hipLaunchKernelGGL(tconv_wgrad_fin_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
        R3D_LAUNCH_CHECK();
    }
    return R3D_OK;
}
