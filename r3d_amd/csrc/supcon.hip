// Supervised contrastive loss (reference loss/spc.py, SupConLoss) as a streaming kernel: N contrast rows z_r of width
// 1 <= D <= 256 (the wide route below: <= 2048), the first A of them anchors, s_ij = z_i . z_j / T, and no N x N tensor in
// memory.
//
//   C(i)   = { j != i : row j is not ignored }          lse_i = log sum_{j in C(i)} exp s_ij
//   Pos(i) = { j in C(i) : y_j = y_i },  P_i = |Pos(i)|
//   l_i    = -(T / T_b) ((1 / P_i) sum_{Pos(i)} s_ij - lse_i)   when P_i > 0, else 0
//   loss   = sum over non-ignored anchors of l_i / max(1, their number n_a)
//
// The maximum of the online log-sum-exp runs over C(i) only: the diagonal |z_i|^2 / T, which the reference subtracts
// and which underflows every other exp on unnormalised rows, never enters.  Row r carries the label of sample r mod bsz
// (the views of a sample are bsz rows apart); labels == NULL is the SimCLR case y = sample index.
//
// Tile discipline of attention_tiled.hip (tile_mma.h): 256 threads, 64 x 64 score tiles, width zero-padded in LDS to
// DP in {16, 32, 64, 128, 256}, fp32-input MFMA chains.  Two operand tiles of 64 x (DP + 4), one score tile and the row /
// column statistics are 150 KiB at DP = 256.
//
//   forward   grid ceil(N / 64): the workgroup of row tile i0 stages it (normalize: divides each row by max(|x|, 1e-12)
//             in LDS and writes 1 / that to the workspace), and if it holds anchors sweeps the column tiles under an online
//             max / sum, with sum_{Pos} s_ij and P_i next to it; writes lse, the positive mean and P per row.
//   finalize  one workgroup: l_i and n_a in a fixed order -> loss_out[0]; n_a is kept in the workspace.
//   backward  grid ceil(N / 64): G_ij = c ([P_i > 0] exp(s_ij - lse_i) - [j in Pos(i)] / P_i) on anchors i, j in C(i), with
//             c = g (T / T_b) / n_a.  s is symmetric, so row tile k0 forms W = G + G^T tile by tile from the statistics of both
//             tiles and accumulates dz_k = (1 / T) sum_j W_kj z_j in one sweep: no second kernel, no atomics.  normalize: the
//             row epilogue applies dx = (dz - z (z . dz)) / |x|.
//
// The wide route (r3d_supcon_wide_*, opt-in; 257 <= D <= 2048, narrower rows make the launches above): the same arithmetic
// with the width walked in chunks of 256 columns, so the LDS footprint is that of DP = 256 plus the two 1 / |x| vectors.
//
//   rinv      one wave per row: 1 / max(|x|, 1e-12) (normalize) or 1 -> the workspace.  The rows are staged raw from here
//             on: s_ij = x_i . x_j rinv_i rinv_j / T, and W's column j carries rinv_j (W z_j = (W rinv_j) x_j).
//   forward   grid ceil(N / 64): per column tile both operand tiles are staged chunk by chunk and the score tile is
//             accumulated in registers before the statistics pass reads it; the sweep and finalize are the ones above.
//   backward  grid (ceil(N / 64), ceil(D / 256)): workgroup (k0, oc) recomputes the full-width score tile per column tile,
//             the chunks in the forward's order (the same bits of s_ij: where lse_i = s_ij, exp(s_ij - lse_i) is 1 as in
//             the narrow pair), fetches chunk oc of the column tile again unless it is the last one, and accumulates
//             columns [256 oc, 256 oc + 256) of dz with it.  Without normalize it writes dx.  normalize: it writes dz to
//             the workspace, and
//   rows      one wave per row forms z . dz over the whole width and writes dx = (dz - z (z . dz)) / |x|.
#include "common.h"
#include "tile_mma.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int SUPCON_MAX_D = 256;
constexpr int SUPCON_WIDE_MAX_D = 2048;
constexpr int WCH = 256;                // the wide route's column chunk (= its DP)

struct SupconArgs {
    const float* x;
    int ld;
    const int64_t* labels;      // [bsz] or NULL
    int bsz, N, A, D;
    int has_ignore;
    int64_t ignore_index;
    float inv_t, t_ratio;       // 1 / T, T / T_b
    int normalize;
    float* ws;                  // lse [N], positive mean [N], P [N], 1 / max(|x|, eps) [N], n_a [1]; wide + normalize: 3 unused,
                                // dz [N][D]
    float* loss_out;
    const float* d_loss;        // upstream gradient (device scalar) or NULL = 1
    float gscale;
    float* dx;
    int lddx, add;
};

__device__ __forceinline__ int64_t row_label(const SupconArgs& a, int r) {
    const int s = r % a.bsz;
    return a.labels ? a.labels[s] : (int64_t)s;
}

// row r is a contrast row: inside the matrix and not ignored
__device__ __forceinline__ bool row_kept(const SupconArgs& a, int r, int64_t y) {
    return r < a.N && !(a.has_ignore && a.labels && y == a.ignore_index);
}

// Row srow of an LDS operand tile, 4 lanes per row (lane `part` takes columns part, part + 4, ...: 8 rows x 4 lanes of a
// half wave hit 32 distinct banks).
template <int DP>
__device__ __forceinline__ void scale_row(float* Z, int srow, int part, float f) {
    float* zp = Z + srow * (DP + 4);
#pragma unroll 8
    for (int d = part; d < DP; d += 4) zp[d] *= f;
}

template <int DP>
__device__ __forceinline__ float unit_row(float* Z, int srow, int part) {        // F.normalize(x, dim=1); returns 1 / max(|x|, eps)
    const float* zp = Z + srow * (DP + 4);
    float ss = 0.f;
#pragma unroll 8
    for (int d = part; d < DP; d += 4) ss += zp[d] * zp[d];
    const float inv = 1.0f / fmaxf(sqrtf(quad_sum(ss)), 1e-12f);
    scale_row<DP>(Z, srow, part, inv);
    return inv;
}

struct SupconLds {
    float *Zi, *Zj, *Ss, *rowl, *rowip, *coll, *colip;
    int64_t *rowy, *coly;
    int *rowok, *colok;
    float *rowri, *colri;       // the wide route only: 1 / max(|x|, eps) of the tile's rows and columns
};

template <int DP>
__device__ __forceinline__ SupconLds supcon_lds(float* lds) {
    constexpr int LD = DP + 4;
    SupconLds s;
    s.Zi = lds;                         // [64][LD]
    s.Zj = s.Zi + TT * LD;              // [64][LD]
    s.Ss = s.Zj + TT * LD;              // [64][SLD]
    s.rowl = s.Ss + TT * SLD;           // [64] each: lse (+inf: no gradient from this row as an anchor), 1 / P (or 0)
    s.rowip = s.rowl + TT;
    s.coll = s.rowip + TT;
    s.colip = s.coll + TT;
    s.rowy = reinterpret_cast<int64_t*>(s.colip + TT);      // (an even number of floats precedes: 8-byte aligned)
    s.coly = s.rowy + TT;
    s.rowok = reinterpret_cast<int*>(s.coly + TT);
    s.colok = s.rowok + TT;
    s.rowri = reinterpret_cast<float*>(s.colok + TT);
    s.colri = s.rowri + TT;
    return s;
}

static size_t supcon_lds_bytes(int dp) {                       // (without rowri / colri)
    return ((size_t)2 * TT * (dp + 4) + (size_t)TT * SLD + 4 * TT) * sizeof(float) + 2 * TT * sizeof(int64_t) + 2 * TT * sizeof(int);
}

template <int DP>
__global__ __launch_bounds__(256) void supcon_fwd_kernel(const SupconArgs a) {
    constexpr int LD = DP + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SupconLds s = supcon_lds<DP>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int N = a.N, A = a.A, D = a.D, i0 = blockIdx.x * TT;
    float *w_lse = a.ws, *w_pm = a.ws + N, *w_P = a.ws + 2 * (size_t)N, *w_rinv = a.ws + 3 * (size_t)N;
    // statistics role: row srow of the tile, columns 4t + part
    const int srow = 16 * w + (lane >> 2), part = lane & 3, gi = i0 + srow;
    stage_tile<DP>(s.Zi, a.x, a.ld, i0, N, D, tid);
    __syncthreads();
    {
        const float inv = a.normalize ? unit_row<DP>(s.Zi, srow, part) : 1.0f;
        if (part == 0 && gi < N) w_rinv[gi] = inv;
    }
    if (i0 >= A) return;                                        // (the whole workgroup: a tile without anchors)
    const int64_t yi = gi < N ? row_label(a, gi) : 0;
    const bool anchor = gi < A && row_kept(a, gi, yi);
    float m = -INFINITY, l = 0.f, psum = 0.f, pcnt = 0.f;
    for (int j0 = 0; j0 < N; j0 += TT) {
        __syncthreads();                                        // the previous tile's readers are done with Zj / Ss / col*
        stage_tile<DP>(s.Zj, a.x, a.ld, j0, N, D, tid);
        if (tid < TT) {
            const int j = j0 + tid;
            const int64_t y = j < N ? row_label(a, j) : 0;
            s.coly[tid] = y;
            s.colok[tid] = row_kept(a, j, y) ? 1 : 0;
        }
        __syncthreads();
        if (a.normalize) {
            unit_row<DP>(s.Zj, srow, part);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(sc, s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) s.Ss[(16 * w + 4 * kq + r) * SLD + 16 * t + c] = sc[r] * a.inv_t;
        }
        __syncthreads();
        float sv[16], mx = -INFINITY;
        bool in_c[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = 4 * t + part;
            sv[t] = s.Ss[srow * SLD + col];
            in_c[t] = s.colok[col] && j0 + col != gi;
            if (in_c[t]) mx = fmaxf(mx, sv[t]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        const float m_new = fmaxf(m, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;   // nothing admissible so far: exp(-inf - 0) = 0, not NaN
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            if (!in_c[t]) continue;
            sum += expf(sv[t] - m_use);
            if (s.coly[4 * t + part] == yi) {
                psum += sv[t];
                pcnt += 1.0f;
            }
        }
        l = l * expf(m - m_use) + quad_sum(sum);
        m = m_new;
    }
    psum = quad_sum(psum);
    pcnt = quad_sum(pcnt);
    if (part == 0 && gi < A) {
        const bool act = anchor && pcnt > 0.f;
        w_lse[gi] = l > 0.f ? m + logf(l) : 0.f;                 // no admissible contrast: the row contributes 0
        w_pm[gi] = act ? psum / pcnt : 0.f;
        w_P[gi] = act ? pcnt : 0.f;
    }
}

__global__ __launch_bounds__(256) void supcon_finalize_kernel(const SupconArgs a) {
    __shared__ double ssum[256];
    __shared__ int scnt[256];
    const int tid = threadIdx.x, N = a.N;
    const float *w_lse = a.ws, *w_pm = a.ws + N, *w_P = a.ws + 2 * (size_t)N;
    double sum = 0.0;
    int cnt = 0;
    for (int i = tid; i < a.A; i += 256) {
        if (!row_kept(a, i, row_label(a, i))) continue;
        ++cnt;
        if (w_P[i] > 0.f) sum -= (double)a.t_ratio * ((double)w_pm[i] - (double)w_lse[i]);
    }
    ssum[tid] = sum;
    scnt[tid] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            ssum[tid] += ssum[tid + h];
            scnt[tid] += scnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int n_a = scnt[0] > 1 ? scnt[0] : 1;
        a.loss_out[0] = (float)(ssum[0] / (double)n_a);
        a.ws[4 * (size_t)N] = (float)n_a;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void supcon_bwd_kernel(const SupconArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SupconLds s = supcon_lds<DP>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int N = a.N, A = a.A, D = a.D, k0 = blockIdx.x * TT;
    const float *w_lse = a.ws, *w_P = a.ws + 2 * (size_t)N, *w_rinv = a.ws + 3 * (size_t)N;
    const int srow = 16 * w + (lane >> 2), part = lane & 3;
    // c / T: every entry of W carries it, so the accumulators are dz itself
    const float coef = (a.d_loss ? a.d_loss[0] : 1.0f) * a.gscale * a.t_ratio / a.ws[4 * (size_t)N] * a.inv_t;
    stage_tile<DP>(s.Zi, a.x, a.ld, k0, N, D, tid);
    if (tid < TT) {
        const int r = k0 + tid;
        const int64_t y = r < N ? row_label(a, r) : 0;
        const bool kept = row_kept(a, r, y);
        const float P = (kept && r < A) ? w_P[r] : 0.f;
        s.rowy[tid] = y;
        s.rowok[tid] = kept ? 1 : 0;
        s.rowl[tid] = P > 0.f ? w_lse[r] : INFINITY;
        s.rowip[tid] = P > 0.f ? 1.0f / P : 0.f;
    }
    __syncthreads();
    if (a.normalize) scale_row<DP>(s.Zi, srow, part, k0 + srow < N ? w_rinv[k0 + srow] : 0.f);
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < N; j0 += TT) {
        if (k0 >= A && j0 >= A) break;                          // neither tile holds an anchor: W = 0 from here on
        __syncthreads();
        stage_tile<DP>(s.Zj, a.x, a.ld, j0, N, D, tid);
        if (tid < TT) {
            const int r = j0 + tid;
            const int64_t y = r < N ? row_label(a, r) : 0;
            const bool kept = row_kept(a, r, y);
            const float P = (kept && r < A) ? w_P[r] : 0.f;
            s.coly[tid] = y;
            s.colok[tid] = kept ? 1 : 0;
            s.coll[tid] = P > 0.f ? w_lse[r] : INFINITY;
            s.colip[tid] = P > 0.f ? 1.0f / P : 0.f;
        }
        __syncthreads();
        if (a.normalize) {
            scale_row<DP>(s.Zj, srow, part, j0 + srow < N ? w_rinv[j0 + srow] : 0.f);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(sc, s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
            const int col = 16 * t + c;
            const float cl = s.coll[col], cip = s.colip[col];
            const int64_t cy = s.coly[col];
            const bool cok = s.colok[col] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                const float sij = sc[r] * a.inv_t;
                float g = 0.f;
                if (cok && s.rowok[row] && k0 + row != j0 + col) {
                    const float eq = s.rowy[row] == cy ? 1.0f : 0.f;
                    g = (expf(sij - s.rowl[row]) - eq * s.rowip[row]) + (expf(sij - cl) - eq * cip);      // G_kj + G_jk
                }
                s.Ss[row * SLD + col] = g * coef;
            }
        }
        __syncthreads();
        mma_nn<DP>(acc, s.Ss + 16 * w * SLD, s.Zj, c, kq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * w + 4 * kq + r, gk = k0 + row;
        if (a.normalize) {                                      // dx = (dz - z (z . dz)) / |x|
            float dot = 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) dot += acc[n][r] * s.Zi[row * LD + 16 * n + c];
            dot += __shfl_xor(dot, 1);
            dot += __shfl_xor(dot, 2);
            dot += __shfl_xor(dot, 4);
            dot += __shfl_xor(dot, 8);
            const float rin = gk < N ? w_rinv[gk] : 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n][r] = (acc[n][r] - s.Zi[row * LD + 16 * n + c] * dot) * rin;
        }
        if (gk >= N) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if (16 * n + c >= D) continue;
            float* p = a.dx + (size_t)gk * a.lddx + 16 * n + c;
            *p = a.add ? *p + acc[n][r] : acc[n][r];
        }
    }
}

// ---- the wide route: 257 <= D <= 2048 in chunks of WCH columns ---------------------------------------------------------

static size_t supcon_wide_lds_bytes() { return supcon_lds_bytes(WCH) + 2 * TT * sizeof(float); }

static int supcon_nchunk(int D) { return r3d_cdiv(D, WCH); }

// supcon_fwd_kernel's running statistics of row gi and its pass over a score tile, as they stand there (statistics role: row
// srow of the tile, 4 lanes, columns 4t + part).  Restated for the wide kernels, like stage_stats below, and not shared
// with the narrow ones, so that those compile to the instruction streams they had.
struct RowStats {
    float m = -INFINITY, l = 0.f, psum = 0.f, pcnt = 0.f;

    // the score tile of column tile j0 is in Ss, its labels and kept flags in coly / colok
    __device__ __forceinline__ void step(const SupconLds& s, int srow, int part, int gi, int j0, int64_t yi) {
        float sv[16], mx = -INFINITY;
        bool in_c[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = 4 * t + part;
            sv[t] = s.Ss[srow * SLD + col];
            in_c[t] = s.colok[col] && j0 + col != gi;
            if (in_c[t]) mx = fmaxf(mx, sv[t]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        const float m_new = fmaxf(m, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;   // nothing admissible so far: exp(-inf - 0) = 0, not NaN
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            if (!in_c[t]) continue;
            sum += expf(sv[t] - m_use);
            if (s.coly[4 * t + part] == yi) {
                psum += sv[t];
                pcnt += 1.0f;
            }
        }
        l = l * expf(m - m_use) + quad_sum(sum);
        m = m_new;
    }

    // after the sweep: lse, the positive mean and P of row gi -> the workspace
    __device__ __forceinline__ void store(const SupconArgs& a, int part, int gi, bool anchor) {
        psum = quad_sum(psum);
        pcnt = quad_sum(pcnt);
        if (part == 0 && gi < a.A) {
            const bool act = anchor && pcnt > 0.f;
            a.ws[gi] = l > 0.f ? m + logf(l) : 0.f;                           // no admissible contrast: the row contributes 0
            a.ws[(size_t)a.N + gi] = act ? psum / pcnt : 0.f;
            a.ws[2 * (size_t)a.N + gi] = act ? pcnt : 0.f;
        }
    }
};

// What the backward needs of row r as a row or a column of W, as supcon_bwd_kernel stages it: label, kept flag, lse (+inf:
// no gradient from this row as an anchor) and 1 / P (or 0).
__device__ __forceinline__ void stage_stats(const SupconArgs& a, int r, int64_t* y_out, int* ok, float* lse, float* ip) {
    const float *w_lse = a.ws, *w_P = a.ws + 2 * (size_t)a.N;
    const int64_t y = r < a.N ? row_label(a, r) : 0;
    const bool kept = row_kept(a, r, y);
    const float P = (kept && r < a.A) ? w_P[r] : 0.f;
    *y_out = y;
    *ok = kept ? 1 : 0;
    *lse = P > 0.f ? w_lse[r] : INFINITY;
    *ip = P > 0.f ? 1.0f / P : 0.f;
}

// the backward's staging area behind the statistics (normalize): dz [N][D]
__device__ __forceinline__ float* wide_dz(const SupconArgs& a) { return a.ws + 4 * (size_t)a.N + 4; }

// One wave per row: ws rinv[r] = 1 / max(|x_r|, 1e-12) (normalize) or 1.
__global__ __launch_bounds__(256) void supcon_rinv_kernel(const SupconArgs a) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.N) return;
    float inv = 1.0f;
    if (a.normalize) {
        const float* xp = a.x + (size_t)r * a.ld;
        float ss = 0.f;
        for (int d = lane; d < a.D; d += 64) ss += xp[d] * xp[d];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) ss += __shfl_xor(ss, o);
        inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    if (lane == 0) a.ws[3 * (size_t)a.N + r] = inv;
}

// chunk [c0, c0 + WCH) of the rows of tiles i0 and j0 -> Zi, Zj
__device__ __forceinline__ void stage_chunk_pair(const SupconLds& s, const SupconArgs& a, int i0, int j0, int c0, int tid) {
    stage_tile<WCH>(s.Zi, a.x + c0, a.ld, i0, a.N, a.D - c0, tid);
    stage_tile<WCH>(s.Zj, a.x + c0, a.ld, j0, a.N, a.D - c0, tid);
}

__global__ __launch_bounds__(256) void supcon_wide_fwd_kernel(const SupconArgs a) {
    constexpr int LD = WCH + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SupconLds s = supcon_lds<WCH>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int N = a.N, A = a.A, D = a.D, i0 = blockIdx.x * TT;
    const float* w_rinv = a.ws + 3 * (size_t)N;
    const int srow = 16 * w + (lane >> 2), part = lane & 3, gi = i0 + srow;
    if (i0 >= A) return;                                        // (the whole workgroup: a tile without anchors)
    const int64_t yi = gi < N ? row_label(a, gi) : 0;
    const bool anchor = gi < A && row_kept(a, gi, yi);
    if (tid < TT) s.rowri[tid] = i0 + tid < N ? w_rinv[i0 + tid] : 0.f;
    RowStats st;
    for (int j0 = 0; j0 < N; j0 += TT) {
        f32x4 sc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < D; c0 += WCH) {
            __syncthreads();                                    // the previous chunk's / tile's readers are done with Zi / Zj / Ss / col*
            stage_chunk_pair(s, a, i0, j0, c0, tid);
            if (c0 == 0 && tid < TT) {
                const int j = j0 + tid;
                const int64_t y = j < N ? row_label(a, j) : 0;
                s.coly[tid] = y;
                s.colok[tid] = row_kept(a, j, y) ? 1 : 0;
                s.colri[tid] = j < N ? w_rinv[j] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 4; ++t) mma_nt<WCH>(sc[t], s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float cs = s.colri[16 * t + c] * a.inv_t;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                s.Ss[row * SLD + 16 * t + c] = sc[t][r] * s.rowri[row] * cs;
            }
        }
        __syncthreads();
        st.step(s, srow, part, gi, j0, yi);
    }
    st.store(a, part, gi, anchor);
}

__global__ __launch_bounds__(256) void supcon_wide_bwd_kernel(const SupconArgs a) {
    constexpr int LD = WCH + 4, NT = WCH / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SupconLds s = supcon_lds<WCH>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int N = a.N, A = a.A, D = a.D, k0 = blockIdx.x * TT;
    const int oc = blockIdx.y, nch = gridDim.y, oc0 = oc * WCH;  // this workgroup's columns of dz: [oc0, oc0 + WCH)
    const float* w_rinv = a.ws + 3 * (size_t)N;
    const float coef = (a.d_loss ? a.d_loss[0] : 1.0f) * a.gscale * a.t_ratio / a.ws[4 * (size_t)N] * a.inv_t;
    if (tid < TT) {
        stage_stats(a, k0 + tid, s.rowy + tid, s.rowok + tid, s.rowl + tid, s.rowip + tid);
        s.rowri[tid] = k0 + tid < N ? w_rinv[k0 + tid] : 0.f;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < N; j0 += TT) {
        if (k0 >= A && j0 >= A) break;                          // neither tile holds an anchor: W = 0 from here on
        f32x4 sc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < D; c0 += WCH) {                   // (the forward's order: the same bits of s_ij, so exp(s - lse)
            __syncthreads();                                    //  is what the forward summed)
            stage_chunk_pair(s, a, k0, j0, c0, tid);
            if (c0 == 0 && tid < TT) {
                stage_stats(a, j0 + tid, s.coly + tid, s.colok + tid, s.coll + tid, s.colip + tid);
                s.colri[tid] = j0 + tid < N ? w_rinv[j0 + tid] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 4; ++t) mma_nt<WCH>(sc[t], s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
        }
        if (oc != nch - 1) {                                    // (the whole workgroup) Zj holds the last chunk: fetch chunk oc
            __syncthreads();
            stage_tile<WCH>(s.Zj, a.x + oc0, a.ld, j0, N, D - oc0, tid);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 16 * t + c;
            const float cl = s.coll[col], cip = s.colip[col], cri = s.colri[col];
            const int64_t cy = s.coly[col];
            const bool cok = s.colok[col] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r;
                const float sij = sc[t][r] * s.rowri[row] * (cri * a.inv_t);
                float g = 0.f;
                if (cok && s.rowok[row] && k0 + row != j0 + col) {
                    const float eq = s.rowy[row] == cy ? 1.0f : 0.f;
                    g = (expf(sij - s.rowl[row]) - eq * s.rowip[row]) + (expf(sij - cl) - eq * cip);      // G_kj + G_jk
                }
                s.Ss[row * SLD + col] = g * coef * cri;         // (Zj holds x_j, not z_j)
            }
        }
        __syncthreads();
        mma_nn<WCH>(acc, s.Ss + 16 * w * SLD, s.Zj, c, kq);
    }
    float* dzs = wide_dz(a);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * w + 4 * kq + r, gk = k0 + row;
        if (gk >= N) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = oc0 + 16 * n + c;
            if (col >= D) continue;
            if (a.normalize) {
                dzs[(size_t)gk * D + col] = acc[n][r];
            } else {
                float* p = a.dx + (size_t)gk * a.lddx + col;
                *p = a.add ? *p + acc[n][r] : acc[n][r];
            }
        }
    }
}

// normalize: one wave per row, dx = (dz - z (z . dz)) / |x| with z = x rinv
__global__ __launch_bounds__(256) void supcon_wide_rows_kernel(const SupconArgs a) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.N) return;
    const float* dz = wide_dz(a) + (size_t)r * a.D;
    const float* xp = a.x + (size_t)r * a.ld;
    const float rin = a.ws[3 * (size_t)a.N + r];
    float dot = 0.f;
    for (int d = lane; d < a.D; d += 64) dot += dz[d] * xp[d];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) dot += __shfl_xor(dot, o);
    dot *= rin;
    for (int d = lane; d < a.D; d += 64) {
        const float v = (dz[d] - xp[d] * rin * dot) * rin;
        float* p = a.dx + (size_t)r * a.lddx + d;
        *p = a.add ? *p + v : v;
    }
}

// The widths the pair runs: the single statement of its limit (r3d_supcon_supported, and both launches).
static bool supcon_width_ok(int D) { return D >= 1 && D <= SUPCON_MAX_D; }

static bool supcon_wide_width_ok(int D) { return D >= 1 && D <= SUPCON_WIDE_MAX_D; }

static int supcon_check(const SupconArgs& a, bool bwd, bool wide = false) {
    if (!(wide ? supcon_wide_width_ok(a.D) : supcon_width_ok(a.D)) || a.N < 1 || a.A < 1 || a.A > a.N || a.bsz < 1 || a.N % a.bsz) return R3D_EINVAL;
    if (!a.x || !a.ws || a.ld < a.D) return R3D_EINVAL;
    if (!(a.inv_t > 0.f) || !(a.t_ratio > 0.f)) return R3D_EINVAL;
    if (!bwd && !a.loss_out) return R3D_EINVAL;
    if (bwd && (!a.dx || a.lddx < a.D)) return R3D_EINVAL;
    return R3D_OK;
}

template <int DP>
static int supcon_launch(const SupconArgs& a, bool bwd, hipStream_t s) {
    const size_t lds = supcon_lds_bytes(DP);
    const dim3 grid(r3d_cdiv(a.N, TT)), blk(256);
    hipError_t e = allow_dynamic_lds(bwd ? (const void*)supcon_bwd_kernel<DP> : (const void*)supcon_fwd_kernel<DP>, lds);
    if (e != hipSuccess) return (int)e;
    if (bwd) {
        hipLaunchKernelGGL(supcon_bwd_kernel<DP>, grid, blk, lds, s, a);
        R3D_LAUNCH_CHECK();
        return R3D_OK;
    }
    hipLaunchKernelGGL(supcon_fwd_kernel<DP>, grid, blk, lds, s, a);
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_finalize_kernel, dim3(1), blk, 0, s, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

static int supcon_dispatch(const SupconArgs& a, bool bwd, void* stream) {
    int rc = supcon_check(a, bwd);
    if (rc != R3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (tile_dp(a.D)) {
        case 16: return supcon_launch<16>(a, bwd, s);
        case 32: return supcon_launch<32>(a, bwd, s);
        case 64: return supcon_launch<64>(a, bwd, s);
        case 128: return supcon_launch<128>(a, bwd, s);
        default: return supcon_launch<256>(a, bwd, s);
    }
}

// The wide entries: D <= 256 makes the launches above.
static int supcon_wide_dispatch(const SupconArgs& a, bool bwd, void* stream) {
    if (a.D <= SUPCON_MAX_D) return supcon_dispatch(a, bwd, stream);
    int rc = supcon_check(a, bwd, true);
    if (rc != R3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = supcon_wide_lds_bytes();
    const int nch = supcon_nchunk(a.D);
    const dim3 tiles(r3d_cdiv(a.N, TT)), rows(r3d_cdiv(a.N, 4)), blk(256);
    hipError_t e = hipFuncSetAttribute(bwd ? (const void*)supcon_wide_bwd_kernel : (const void*)supcon_wide_fwd_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    if (bwd) {
        hipLaunchKernelGGL(supcon_wide_bwd_kernel, dim3(tiles.x, nch), blk, lds, s, a);
        R3D_LAUNCH_CHECK();
        if (a.normalize) {
            hipLaunchKernelGGL(supcon_wide_rows_kernel, rows, blk, 0, s, a);
            R3D_LAUNCH_CHECK();
        }
        return R3D_OK;
    }
    hipLaunchKernelGGL(supcon_rinv_kernel, rows, blk, 0, s, a);
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_wide_fwd_kernel, tiles, blk, lds, s, a);
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_finalize_kernel, dim3(1), blk, 0, s, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

static SupconArgs supcon_args(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                              int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws) {
    SupconArgs a{};
    a.x = x; a.ld = ldx; a.labels = labels; a.bsz = bsz; a.N = N; a.A = A; a.D = D;
    a.has_ignore = has_ignore; a.ignore_index = ignore_index;
    a.inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    a.t_ratio = base_temperature > 0.f ? temperature / base_temperature : 0.f;
    a.normalize = normalize; a.ws = ws;
    return a;
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_supcon_supported(int D) { return supcon_width_ok(D) ? 1 : 0; }

R3D_EXPORT int64_t r3d_supcon_ws_floats(int N) { return N >= 1 ? 4 * (int64_t)N + 4 : 0; }

R3D_EXPORT int r3d_supcon_fwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                              int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                              float* loss_out, void* stream) {
    SupconArgs a = supcon_args(x, ldx, labels, bsz, N, A, D, has_ignore, ignore_index, temperature, base_temperature, normalize, ws);
    a.loss_out = loss_out;
    return supcon_dispatch(a, false, stream);
}

R3D_EXPORT int r3d_supcon_bwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                              int64_t ignore_index, float temperature, float base_temperature, int normalize, const float* ws,
                              const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream) {
    SupconArgs a = supcon_args(x, ldx, labels, bsz, N, A, D, has_ignore, ignore_index, temperature, base_temperature, normalize,
                               const_cast<float*>(ws));
    a.d_loss = d_loss; a.gscale = gscale; a.dx = dx; a.lddx = lddx; a.add = add;
    return supcon_dispatch(a, true, stream);
}

R3D_EXPORT int r3d_supcon_wide_supported(int D) { return supcon_wide_width_ok(D) ? 1 : 0; }

R3D_EXPORT int64_t r3d_supcon_wide_ws_floats(int N, int D, int normalize) {
    if (N < 1 || !supcon_wide_width_ok(D)) return 0;
    const int64_t stats = 4 * (int64_t)N + 4;
    return normalize && D > SUPCON_MAX_D ? stats + (int64_t)N * D : stats;
}

R3D_EXPORT int r3d_supcon_wide_fwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                                   int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                                   float* loss_out, void* stream) {
    SupconArgs a = supcon_args(x, ldx, labels, bsz, N, A, D, has_ignore, ignore_index, temperature, base_temperature, normalize, ws);
    a.loss_out = loss_out;
    return supcon_wide_dispatch(a, false, stream);
}

R3D_EXPORT int r3d_supcon_wide_bwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                                   int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                                   const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream) {
    SupconArgs a = supcon_args(x, ldx, labels, bsz, N, A, D, has_ignore, ignore_index, temperature, base_temperature, normalize, ws);
    a.d_loss = d_loss; a.gscale = gscale; a.dx = dx; a.lddx = lddx; a.add = add;
    return supcon_wide_dispatch(a, true, stream);
}
