// The reference's temporal auxiliary objectives (utils.py: temporal_contrastive_loss :229, temporal_cluster_loss :271,
// focal_loss :493) and the run detection they are fed by (train/train_unsupervised.py: get_cluster_intervals :34).
//
// Runs.  A run of clip b starts at t = 0 and wherever labels[b, t] != labels[b, t - 1].  r3d_label_runs writes per frame
// the first and last frame of its run, per clip the run count and the compact list of run starts: one launch, one
// workgroup per clip, every thread a contiguous chunk of frames, the chunks joined through LDS.
//
// Cluster loss.  Run r of clip b: n_r frames, mean m_r.
//   intra = sum_{b,r} (1 / (n_r C)) sum_{t in r, c} (x - m_r)^2 / total            total = runs in the batch
//   inter = sum_{b: R_b > 1} sum_{i<j} 1 / (1e-5 + |m_i - m_j|) / (M (n_last - 1))  M = clips with R_b > 1, n_last = R of the
//                                                                                  last of them
//   means     a wave per run: mean and the run's intra term.
//   pairs     32 x 32 tiles of (i, j) run pairs per clip, the two mean tiles in LDS, the difference formed directly in
//             fp32 (no Gram expansion: 1 / (1e-5 + d) amplifies its cancellation); one partial per tile.
//   finalize  one workgroup: every partial in a fixed order -> loss; 1 / total and 1 / (M (n_last - 1)) stay in ws.
//   backward  a wave per run: dm_i = -sum_{j != i} (m_i - m_j) / (d (1e-5 + d)^2) (0 where d = 0), spread as dm / n_r over the
//             run's frames next to 2 (x - m) / (n_r C total).
//
// Contrastive loss.  Per clip z = x / max(|x|, 1e-12), s = z z^T / tau, p = softmax over every column (self included).  Frame
// t of run (st, en): P(t) = { c : st <= c <= en, c != t - st } (the reference's fill_diagonal_ on its [n, T] mask removes
// the row's index inside its run, not t).  loss = sum_b sum_r sum_{t in r} sum_{P(t)} -log(p + 1e-5) / (|P_r| + 1e-5) / B.
// Tile discipline of supcon.hip (tile_mma.h), one workgroup per (clip, 64-row tile), no [T, T] tensor:
//   forward   pass 1: online max / sum over all column tiles -> lse.  pass 2: only the column tiles that meet the tile's
//             runs: the loss terms and Q_t = sum_{P(t)} q, q = p / (p + 1e-5).  Keeps lse, Q, 1 / |x|, |x| and the row's term.
//   finalize  one workgroup: the rows' terms in a fixed order.
//   backward  dL/ds_tc = -w_t (q_tc [c in P(t)] - p_tc Q_t), w_t = g / (B (|P_r| + 1e-5)); s is symmetric, so row tile I forms
//             G_IJ + G_JI^T per column tile from the statistics of both and accumulates dz_I in one sweep; the row epilogue
//             applies dx = (dz - z (z . dz)) / max(|x|, 1e-12).
//
// Focal loss.  A wave per row of pred [N, C]: lse, argmax, CE = lse - x_gold, p = exp(-CE),
//   row = alpha (1 - p)^gamma CE + penalty [argmax == pad], masked rows (gold = pad, = exclude, or outside [0, C)) 0;
//   d row / d x_c = A ([c == gold] - p_c), A = -alpha (gamma (1 - p)^(gamma - 1) CE p + (1 - p)^gamma).
// The same launch writes the gradient and the argmax == gold flags; a one-workgroup finalize sums the rows (mean over all
// N) and the two counters.
//
// Every launch: enqueue only, no allocation, no atomics, reductions in a fixed order.
#include "common.h"
#include "tile_mma.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int TEMPORAL_MAX_W = 256;     // widest row of the cluster (C) and contrastive (D) kernels
constexpr float TEMPORAL_EPS = 1e-5f;   // the reference's 1e-5, in all three places it appears

// sum of 256 per-thread doubles in a fixed order; every thread returns the total
__device__ __forceinline__ double block_sum_d(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// runs of equal labels
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void label_runs_kernel(const int64_t* __restrict__ labels, int T, int* __restrict__ first,
                                                          int* __restrict__ last, int* __restrict__ starts,
                                                          int* __restrict__ count) {
    __shared__ int s_nb[256], s_last[256], s_first[256];
    const int tid = threadIdx.x;
    const size_t off = (size_t)blockIdx.x * T;
    const int64_t* lab = labels + off;
    const int chunk = (T + 255) / 256;
    const int t0 = min(T, tid * chunk), t1 = min(T, t0 + chunk);
    int nb = 0, lb = -1, fb = T;                                // boundaries in the chunk: number, last, first
    for (int t = t0; t < t1; ++t) {
        if (t == 0 || lab[t] != lab[t - 1]) {
            if (nb == 0) fb = t;
            lb = t;
            ++nb;
        }
    }
    s_nb[tid] = nb;
    s_last[tid] = lb;
    s_first[tid] = fb;
    __syncthreads();
    int before = 0, cur = -1, nxt = T, total = 0;
    for (int u = 0; u < 256; ++u) {
        const int n = s_nb[u];
        if (u < tid) {
            before += n;
            if (n) cur = s_last[u];
        }
        if (u > tid && n && nxt == T) nxt = s_first[u];
        total += n;
    }
    int rid = before - 1;
    for (int t = t0; t < t1; ++t) {
        if (t == 0 || lab[t] != lab[t - 1]) {
            cur = t;
            ++rid;
            starts[off + rid] = t;
        }
        first[off + t] = cur;
    }
    for (int t = t1 - 1; t >= t0; --t) {
        last[off + t] = nxt - 1;
        if (t == 0 || lab[t] != lab[t - 1]) nxt = t;
    }
    for (int r = total + tid; r < T; r += 256) starts[off + r] = T;      // past the last run: T
    if (tid == 0) count[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------------------------------
// cluster loss
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PT = 32;                  // run pairs are tiled PT x PT

struct TcluArgs {
    const float* x;
    int ld, B, T, C;
    const int *starts, *last, *count;
    float* ws;                          // means [B T C], intra [B T], pair partials [B nt nt], 1 / total, 1 / (M (n_last - 1))
    float* loss_out;
    const float* d_loss;
    float gscale;
    float* dx;
    int lddx, add;
};

__host__ __device__ __forceinline__ int tclu_nt(int T) { return (T + PT - 1) / PT; }
__host__ __device__ __forceinline__ size_t tclu_off_intra(int B, int T, int C) { return (size_t)B * T * C; }
__host__ __device__ __forceinline__ size_t tclu_off_part(int B, int T, int C) { return tclu_off_intra(B, T, C) + (size_t)B * T; }
__host__ __device__ __forceinline__ size_t tclu_off_scal(int B, int T, int C) {
    return tclu_off_part(B, T, C) + (size_t)B * tclu_nt(T) * tclu_nt(T);
}

// a wave per run: lane l holds columns l, l + 64, l + 128, l + 192
__global__ __launch_bounds__(256) void tclu_means_kernel(const TcluArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y, T = a.T, C = a.C;
    const int r = blockIdx.x * 4 + w;
    if (r >= a.count[b]) return;
    const size_t row0 = (size_t)b * T;
    const int st = a.starts[row0 + r], en = a.last[row0 + st], n = en - st + 1;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = st; t <= en; ++t) {
        const float* xp = a.x + (row0 + t) * a.ld;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) sum[k] += xp[c];
        }
    }
    const float inv_n = 1.0f / (float)n;
    float* mp = a.ws + (row0 + r) * C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sum[k] *= inv_n;
        const int c = lane + 64 * k;
        if (c < C) mp[c] = sum[k];
    }
    float ss = 0.f;
    for (int t = st; t <= en; ++t) {
        const float* xp = a.x + (row0 + t) * a.ld;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                const float d = xp[c] - sum[k];
                ss += d * d;
            }
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) a.ws[tclu_off_intra(a.B, T, C) + row0 + r] = ss / ((float)n * (float)C);
}

// tile (it <= jt) of clip b: sum over its pairs i < j of 1 / (1e-5 + |m_i - m_j|)
__global__ __launch_bounds__(256) void tclu_pairs_kernel(const TcluArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[256];
    const int tid = threadIdx.x, it = blockIdx.x, jt = blockIdx.y, b = blockIdx.z, T = a.T, C = a.C, LD = C + 1;
    const int cnt = a.count[b], i0 = it * PT, j0 = jt * PT, nt = tclu_nt(T);
    if (it > jt || j0 >= cnt || cnt < 2) return;                // (the whole workgroup; the finalize reads live tiles only)
    float *Mi = lds, *Mj = lds + PT * LD;
    const float* means = a.ws + (size_t)b * T * C;
    for (int e = tid; e < PT * C; e += 256) {
        const int r = e / C, c = e % C;
        Mi[r * LD + c] = i0 + r < cnt ? means[(size_t)(i0 + r) * C + c] : 0.f;
        Mj[r * LD + c] = j0 + r < cnt ? means[(size_t)(j0 + r) * C + c] : 0.f;
    }
    __syncthreads();
    const int i = tid >> 3, gi = i0 + i;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = (tid & 7) + 8 * q, gj = j0 + j;
        if (gi >= gj || gj >= cnt) continue;
        float ss = 0.f;
        for (int c = 0; c < C; ++c) {
            const float d = Mi[i * LD + c] - Mj[j * LD + c];
            ss += d * d;
        }
        sum += (double)(1.0f / (TEMPORAL_EPS + sqrtf(ss)));
    }
    sum = block_sum_d(sum, red, tid);
    if (tid == 0) a.ws[tclu_off_part(a.B, T, C) + ((size_t)b * nt + it) * nt + jt] = (float)sum;
}

__global__ __launch_bounds__(256) void tclu_finalize_kernel(const TcluArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x, B = a.B, T = a.T, C = a.C, nt = tclu_nt(T);
    const float* intra = a.ws + tclu_off_intra(B, T, C);
    const float* part = a.ws + tclu_off_part(B, T, C);
    double si = 0.0, se = 0.0;
    for (size_t e = tid; e < (size_t)B * T; e += 256)
        if ((int)(e % T) < a.count[e / T]) si += (double)intra[e];
    si = block_sum_d(si, red, tid);
    long long total = 0;
    int M = 0, n_last = 0;
    for (int b = 0; b < B; ++b) {
        const int cnt = a.count[b];
        total += cnt;
        if (cnt < 2) continue;
        ++M;
        n_last = cnt;
        const int ntb = (cnt + PT - 1) / PT;
        for (int e = tid; e < ntb * ntb; e += 256) {
            const int it = e / ntb, jt = e % ntb;
            if (it <= jt) se += (double)part[((size_t)b * nt + it) * nt + jt];
        }
    }
    se = block_sum_d(se, red, tid);
    if (tid == 0) {
        const double inv_total = total > 0 ? 1.0 / (double)total : 0.0;
        const double inter_scale = M > 0 ? 1.0 / ((double)M * (double)(n_last - 1)) : 0.0;
        float* scal = a.ws + tclu_off_scal(B, T, C);
        scal[0] = (float)inv_total;
        scal[1] = (float)inter_scale;
        if (a.loss_out) a.loss_out[0] = (float)(si * inv_total + se * inter_scale);
    }
}

__global__ __launch_bounds__(256) void tclu_bwd_kernel(const TcluArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y, T = a.T, C = a.C;
    const int r = blockIdx.x * 4 + w, cnt = a.count[b];
    if (r >= cnt) return;
    const size_t row0 = (size_t)b * T;
    const int st = a.starts[row0 + r], en = a.last[row0 + st], n = en - st + 1;
    const float* scal = a.ws + tclu_off_scal(a.B, T, C);
    const float g = (a.d_loss ? a.d_loss[0] : 1.0f) * a.gscale;
    const float* means = a.ws + row0 * C;
    float mi[4], dm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        mi[k] = c < C ? means[(size_t)r * C + c] : 0.f;
        dm[k] = 0.f;
    }
    if (cnt > 1) {
        for (int j = 0; j < cnt; ++j) {
            if (j == r) continue;
            float df[4], ss = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = lane + 64 * k;
                df[k] = c < C ? mi[k] - means[(size_t)j * C + c] : 0.f;
                ss += df[k] * df[k];
            }
            const float d = sqrtf(wave_sum(ss));
            if (d > 0.f) {                                      // d = 0: the subgradient 0 of the norm
                const float e = TEMPORAL_EPS + d, f = 1.0f / (d * e * e);
#pragma unroll
                for (int k = 0; k < 4; ++k) dm[k] -= df[k] * f;
            }
        }
    }
    const float inv_n = 1.0f / (float)n;
    const float ci = g * 2.0f * scal[0] * inv_n / (float)C, ce = g * scal[1] * inv_n;
    for (int t = st; t <= en; ++t) {
        const float* xp = a.x + (row0 + t) * a.ld;
        float* dp = a.dx + (row0 + t) * a.lddx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c >= C) continue;
            const float v = ci * (xp[c] - mi[k]) + ce * dm[k];
            dp[c] = a.add ? dp[c] + v : v;
        }
    }
}

static bool temporal_width_ok(int W) { return W >= 1 && W <= TEMPORAL_MAX_W; }

static bool temporal_rows_ok(int B, int T) { return B >= 1 && T >= 1 && (int64_t)B * T < (int64_t)1 << 30 && B <= 65535; }

static int tclu_check(const TcluArgs& a, bool bwd) {
    if (!temporal_width_ok(a.C) || !temporal_rows_ok(a.B, a.T) || tclu_nt(a.T) > 65535) return R3D_EINVAL;
    if (!a.x || !a.ws || a.ld < a.C || !a.starts || !a.last || !a.count) return R3D_EINVAL;
    if (!bwd && !a.loss_out) return R3D_EINVAL;
    if (bwd && (!a.dx || a.lddx < a.C)) return R3D_EINVAL;
    return R3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// contrastive loss
// ---------------------------------------------------------------------------------------------------------------------
struct TconArgs {
    const float* x;
    int ld, B, T, D;
    const int *first, *last;
    float inv_t;
    float* ws;                          // [B T] each: lse, Q, 1 / max(|x|, 1e-12), the row's loss term, max(|x|, 1e-12)
    float* loss_out;
    const float* d_loss;
    float gscale;
    float* dx;
    int lddx, add;
};

// Rows are divided by their norm, not multiplied by its reciprocal: at D = 1 the quotient is exactly +-1, as F.normalize's,
// and the row epilogue's dz - z (z . dz) is exactly 0 there.
template <int DP>
__device__ __forceinline__ void tcon_divide_row(float* Z, int srow, int part, float nrm) {
    float* zp = Z + srow * (DP + 4);
#pragma unroll 8
    for (int d = part; d < DP; d += 4) zp[d] = zp[d] / nrm;
}

template <int DP>
__device__ __forceinline__ float tcon_unit_row(float* Z, int srow, int part) {   // F.normalize; returns max(|x|, 1e-12)
    const float* zp = Z + srow * (DP + 4);
    float ss = 0.f;
#pragma unroll 8
    for (int d = part; d < DP; d += 4) ss += zp[d] * zp[d];
    const float nrm = fmaxf(sqrtf(quad_sum(ss)), 1e-12f);
    tcon_divide_row<DP>(Z, srow, part, nrm);
    return nrm;
}

// |P_r| of a run (st, en): n^2 minus the in-run "diagonal" entries (i, i), i < n, that fall inside [st, en]
__device__ __forceinline__ float tcon_pairs(int st, int en) {
    const long long n = en - st + 1, cut = n - st;
    return (float)(n * n - (cut > 0 ? cut : 0));
}

struct TconLds {
    float *Zi, *Zj, *Ss, *rowl, *rowq, *roww, *coll, *colq, *colw;
    int *rowst, *rowen, *colst, *colen;
};

template <int DP>
__device__ __forceinline__ TconLds tcon_lds(float* lds) {
    constexpr int LD = DP + 4;
    TconLds s;
    s.Zi = lds;                         // [64][LD]
    s.Zj = s.Zi + TT * LD;              // [64][LD]
    s.Ss = s.Zj + TT * LD;              // [64][SLD]
    s.rowl = s.Ss + TT * SLD;           // [64] each: lse (+inf: a row past T), Q, w; then the run's first and last frame
    s.rowq = s.rowl + TT;
    s.roww = s.rowq + TT;
    s.coll = s.roww + TT;
    s.colq = s.coll + TT;
    s.colw = s.colq + TT;
    s.rowst = reinterpret_cast<int*>(s.colw + TT);
    s.rowen = s.rowst + TT;
    s.colst = s.rowen + TT;
    s.colen = s.colst + TT;
    return s;
}

static size_t tcon_lds_bytes(int dp) { return ((size_t)2 * TT * (dp + 4) + (size_t)TT * SLD + 10 * TT) * sizeof(float); }

// scores of row tile Zi against the column tile starting at j0 -> Ss (normalised rows, / tau)
template <int DP>
__device__ __forceinline__ void tcon_scores(const TconLds& s, const float* xb, const TconArgs& a, int j0, int tid, int srow,
                                            int part) {
    constexpr int LD = DP + 4;
    const int lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    __syncthreads();                                            // the previous tile's readers are done with Zj / Ss
    stage_tile<DP>(s.Zj, xb, a.ld, j0, a.T, a.D, tid);
    __syncthreads();
    tcon_unit_row<DP>(s.Zj, srow, part);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
        mma_nt<DP>(sc, s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
#pragma unroll
        for (int r = 0; r < 4; ++r) s.Ss[(16 * w + 4 * kq + r) * SLD + 16 * t + c] = sc[r] * a.inv_t;
    }
    __syncthreads();
}

template <int DP>
__global__ __launch_bounds__(256) void tcon_fwd_kernel(const TconArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TconLds s = tcon_lds<DP>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int T = a.T, b = blockIdx.y, i0 = blockIdx.x * TT;
    const size_t row0 = (size_t)b * T, BT = (size_t)a.B * T;
    const float* xb = a.x + row0 * a.ld;
    const int srow = 16 * w + (lane >> 2), part = lane & 3, gi = i0 + srow;
    stage_tile<DP>(s.Zi, xb, a.ld, i0, T, a.D, tid);
    __syncthreads();
    const float nrm = tcon_unit_row<DP>(s.Zi, srow, part);
    // pass 1: lse over every column of the clip, self included
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 < T; j0 += TT) {
        tcon_scores<DP>(s, xb, a, j0, tid, srow, part);
        float sv[16], mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = 4 * t + part;
            sv[t] = s.Ss[srow * SLD + col];
            if (j0 + col < T) mx = fmaxf(mx, sv[t]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        const float m_new = fmaxf(m, mx);                       // (finite: every tile of the sweep holds a column < T)
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (j0 + 4 * t + part < T) sum += expf(sv[t] - m_new);
        l = l * expf(m - m_new) + quad_sum(sum);
        m = m_new;
    }
    const float lse = m + logf(l);
    // pass 2: the column tiles that meet the runs of this tile's rows
    const int st = gi < T ? a.first[row0 + gi] : 0, en = gi < T ? a.last[row0 + gi] : -1;
    const int jlo = a.first[row0 + i0] / TT * TT, jhi = a.last[row0 + min(i0 + TT, T) - 1];
    float acc = 0.f, Q = 0.f;
    for (int j0 = jlo; j0 <= jhi; j0 += TT) {
        tcon_scores<DP>(s, xb, a, j0, tid, srow, part);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int gc = j0 + 4 * t + part;
            if (gc < st || gc > en || gc == gi - st) continue;
            const float p = expf(s.Ss[srow * SLD + 4 * t + part] - lse);
            acc -= logf(p + TEMPORAL_EPS);
            Q += p / (p + TEMPORAL_EPS);
        }
    }
    acc = quad_sum(acc);
    Q = quad_sum(Q);
    if (part == 0 && gi < T) {
        a.ws[row0 + gi] = lse;
        a.ws[BT + row0 + gi] = Q;
        a.ws[2 * BT + row0 + gi] = 1.0f / nrm;
        a.ws[3 * BT + row0 + gi] = acc / (tcon_pairs(st, en) + TEMPORAL_EPS);
        a.ws[4 * BT + row0 + gi] = nrm;
    }
}

__global__ __launch_bounds__(256) void tcon_finalize_kernel(const TconArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const size_t BT = (size_t)a.B * a.T;
    const float* term = a.ws + 3 * BT;
    double sum = 0.0;
    for (size_t e = tid; e < BT; e += 256) sum += (double)term[e];
    sum = block_sum_d(sum, red, tid);
    if (tid == 0) a.loss_out[0] = (float)(sum / (double)a.B);
}

template <int DP>
__global__ __launch_bounds__(256) void tcon_bwd_kernel(const TconArgs a) {
    constexpr int LD = DP + 4, NT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TconLds s = tcon_lds<DP>(lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int T = a.T, D = a.D, b = blockIdx.y, k0 = blockIdx.x * TT;
    const size_t row0 = (size_t)b * T, BT = (size_t)a.B * T;
    const float* xb = a.x + row0 * a.ld;
    const float *w_lse = a.ws + row0, *w_q = a.ws + BT + row0, *w_rinv = a.ws + 2 * BT + row0, *w_nrm = a.ws + 4 * BT + row0;
    const int srow = 16 * w + (lane >> 2), part = lane & 3;
    const float coef = (a.d_loss ? a.d_loss[0] : 1.0f) * a.gscale / (float)a.B;
    stage_tile<DP>(s.Zi, xb, a.ld, k0, T, D, tid);
    if (tid < TT) {
        const int r = k0 + tid;
        const bool ok = r < T;
        const int st = ok ? a.first[row0 + r] : 0, en = ok ? a.last[row0 + r] : -1;
        s.rowst[tid] = st;
        s.rowen[tid] = en;
        s.rowl[tid] = ok ? w_lse[r] : INFINITY;
        s.rowq[tid] = ok ? w_q[r] : 0.f;
        s.roww[tid] = ok ? coef / (tcon_pairs(st, en) + TEMPORAL_EPS) : 0.f;
    }
    __syncthreads();
    tcon_divide_row<DP>(s.Zi, srow, part, k0 + srow < T ? w_nrm[k0 + srow] : 1.0f);       // (rows past T are staged as zeros)
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < T; j0 += TT) {
        __syncthreads();
        stage_tile<DP>(s.Zj, xb, a.ld, j0, T, D, tid);
        if (tid < TT) {
            const int r = j0 + tid;
            const bool ok = r < T;
            const int st = ok ? a.first[row0 + r] : 0, en = ok ? a.last[row0 + r] : -1;
            s.colst[tid] = st;
            s.colen[tid] = en;
            s.coll[tid] = ok ? w_lse[r] : INFINITY;
            s.colq[tid] = ok ? w_q[r] : 0.f;
            s.colw[tid] = ok ? coef / (tcon_pairs(st, en) + TEMPORAL_EPS) : 0.f;
        }
        __syncthreads();
        tcon_divide_row<DP>(s.Zj, srow, part, j0 + srow < T ? w_nrm[j0 + srow] : 1.0f);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
            mma_nt<DP>(sc, s.Zi + 16 * w * LD, s.Zj + 16 * t * LD, c, kq);
            const int col = 16 * t + c, gj = j0 + col;
            const float cl = s.coll[col], cq = s.colq[col], cw = s.colw[col];
            const int cst = s.colst[col], cen = s.colen[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * kq + r, gk = k0 + row;
                const float sij = sc[r] * a.inv_t;
                float g = 0.f;
                if (gk < T && gj < T) {
                    const int rst = s.rowst[row];
                    const float pk = expf(sij - s.rowl[row]), pj = expf(sij - cl);
                    const bool in_k = gj >= rst && gj <= s.rowen[row] && gj != gk - rst;     // j in P(k)
                    const bool in_j = gk >= cst && gk <= cen && gk != gj - cst;              // k in P(j)
                    const float gkj = s.roww[row] * (pk * s.rowq[row] - (in_k ? pk / (pk + TEMPORAL_EPS) : 0.f));
                    const float gjk = cw * (pj * cq - (in_j ? pj / (pj + TEMPORAL_EPS) : 0.f));
                    g = (gkj + gjk) * a.inv_t;
                }
                s.Ss[row * SLD + col] = g;
            }
        }
        __syncthreads();
        mma_nn<DP>(acc, s.Ss + 16 * w * SLD, s.Zj, c, kq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * w + 4 * kq + r, gk = k0 + row;
        float dot = 0.f;                                        // dx = (dz - z (z . dz)) / max(|x|, 1e-12)
#pragma unroll
        for (int n = 0; n < NT; ++n) dot += acc[n][r] * s.Zi[row * LD + 16 * n + c];
        dot += __shfl_xor(dot, 1);
        dot += __shfl_xor(dot, 2);
        dot += __shfl_xor(dot, 4);
        dot += __shfl_xor(dot, 8);
        const float rin = gk < T ? w_rinv[gk] : 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n][r] = (acc[n][r] - s.Zi[row * LD + 16 * n + c] * dot) * rin;
        if (gk >= T) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if (16 * n + c >= D) continue;
            float* p = a.dx + (row0 + gk) * a.lddx + 16 * n + c;
            *p = a.add ? *p + acc[n][r] : acc[n][r];
        }
    }
}

static int tcon_check(const TconArgs& a, bool bwd) {
    if (!temporal_width_ok(a.D) || !temporal_rows_ok(a.B, a.T)) return R3D_EINVAL;
    if (!a.x || !a.ws || a.ld < a.D || !a.first || !a.last) return R3D_EINVAL;
    if (!(a.inv_t > 0.f) || !(a.inv_t < INFINITY)) return R3D_EINVAL;
    if (!bwd && !a.loss_out) return R3D_EINVAL;
    if (bwd && (!a.dx || a.lddx < a.D)) return R3D_EINVAL;
    return R3D_OK;
}

template <int DP>
static int tcon_launch(const TconArgs& a, bool bwd, hipStream_t s) {
    const size_t lds = tcon_lds_bytes(DP);
    const dim3 grid(r3d_cdiv(a.T, TT), a.B), blk(256);
    hipError_t e = allow_dynamic_lds(bwd ? (const void*)tcon_bwd_kernel<DP> : (const void*)tcon_fwd_kernel<DP>, lds);
    if (e != hipSuccess) return (int)e;
    if (bwd) {
        hipLaunchKernelGGL(tcon_bwd_kernel<DP>, grid, blk, lds, s, a);
        R3D_LAUNCH_CHECK();
        return R3D_OK;
    }
    hipLaunchKernelGGL(tcon_fwd_kernel<DP>, grid, blk, lds, s, a);
    R3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(tcon_finalize_kernel, dim3(1), blk, 0, s, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

static int tcon_dispatch(const TconArgs& a, bool bwd, void* stream) {
    int rc = tcon_check(a, bwd);
    if (rc != R3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (tile_dp(a.D)) {
        case 16: return tcon_launch<16>(a, bwd, s);
        case 32: return tcon_launch<32>(a, bwd, s);
        case 64: return tcon_launch<64>(a, bwd, s);
        case 128: return tcon_launch<128>(a, bwd, s);
        default: return tcon_launch<256>(a, bwd, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// focal loss
// ---------------------------------------------------------------------------------------------------------------------
struct FocalArgs {
    const float* pred;
    int ld;
    const int64_t* gold;
    int N, C;
    int64_t pad, excl;
    int has_excl;
    float alpha, gamma, penalty;
    float* ws;                          // the rows' loss terms [N]
    float* loss_out;
    uint8_t* flags;
    int64_t* counts;
    const float* d_loss;
    float gscale;
    float* dpred;
    int lddp, add;
};

__device__ __forceinline__ bool focal_row_live(const FocalArgs& a, int64_t g) {
    return g != a.pad && !(a.has_excl && g == a.excl) && g >= 0 && g < a.C;
}

__global__ __launch_bounds__(256) void focal_rows_kernel(const FocalArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, C = a.C;
    const int row = blockIdx.x * 4 + w;
    if (row >= a.N) return;
    const float* xp = a.pred + (size_t)row * a.ld;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = xp[c];
        if (v > best || arg == 0x7fffffff) {
            best = v;
            arg = c;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                          // the largest value, the lowest index among equals
        const float ov = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ov > best || (ov == best && oa < arg))) {
            best = ov;
            arg = oa;
        }
    }
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(xp[c] - best);
    const float lse = best + logf(wave_sum(sum));
    const int64_t g = a.gold[row];
    const bool live = focal_row_live(a, g);
    float term = 0.f, A = 0.f;
    if (live) {
        const float ce = fmaxf(lse - xp[g], 0.f), p = expf(-ce), omp = -expm1f(-ce);
        const float fw = powf(omp, a.gamma);
        term = a.alpha * fw * ce + (arg == a.pad ? a.penalty : 0.f);
        A = -a.alpha * (a.gamma * powf(omp, a.gamma - 1.0f) * ce * p + fw);
    }
    if (lane == 0) {
        if (a.ws) a.ws[row] = term;
        if (a.flags) a.flags[row] = live && arg == g ? 1 : 0;
    }
    if (!a.dpred) return;
    const float f = A * (a.d_loss ? a.d_loss[0] : 1.0f) * a.gscale / (float)a.N;
    float* dp = a.dpred + (size_t)row * a.lddp;
    for (int c = lane; c < C; c += 64) {
        const float v = live ? f * ((c == g ? 1.0f : 0.f) - expf(xp[c] - lse)) : 0.f;
        dp[c] = a.add ? dp[c] + v : v;
    }
}

__global__ __launch_bounds__(256) void focal_finalize_kernel(const FocalArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double sum = 0.0, hit = 0.0, word = 0.0;                    // (counts below 2^53: exact)
    for (int i = tid; i < a.N; i += 256) {
        sum += (double)a.ws[i];
        if (focal_row_live(a, a.gold[i])) {
            word += 1.0;
            if (a.flags[i]) hit += 1.0;
        }
    }
    sum = block_sum_d(sum, red, tid);
    hit = block_sum_d(hit, red, tid);
    word = block_sum_d(word, red, tid);
    if (tid == 0) {
        a.loss_out[0] = (float)(sum / (double)a.N);
        a.counts[0] = (int64_t)hit;
        a.counts[1] = (int64_t)word;
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_label_runs(const int64_t* labels, int B, int T, int* first, int* last, int* starts, int* count,
                              void* stream) {
    if (!labels || !first || !last || !starts || !count || !temporal_rows_ok(B, T)) return R3D_EINVAL;
    hipLaunchKernelGGL(label_runs_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, T, first, last, starts, count);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_temporal_width_supported(int W) { return temporal_width_ok(W) ? 1 : 0; }

R3D_EXPORT int64_t r3d_tcluster_ws_floats(int B, int T, int C) {
    return temporal_rows_ok(B, T) && temporal_width_ok(C) ? (int64_t)tclu_off_scal(B, T, C) + 4 : 0;
}

static TcluArgs tclu_args(const float* x, int ldx, int B, int T, int C, const int* starts, const int* last, const int* count,
                          float* ws) {
    TcluArgs a{};
    a.x = x; a.ld = ldx; a.B = B; a.T = T; a.C = C; a.starts = starts; a.last = last; a.count = count; a.ws = ws;
    return a;
}

R3D_EXPORT int r3d_tcluster_fwd(const float* x, int ldx, int B, int T, int C, const int* starts, const int* last,
                                const int* count, float* ws, float* loss_out, void* stream) {
    TcluArgs a = tclu_args(x, ldx, B, T, C, starts, last, count, ws);
    a.loss_out = loss_out;
    int rc = tclu_check(a, false);
    if (rc != R3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)2 * PT * (C + 1) * sizeof(float);
    if (lds > 48 * 1024) {                                      // (the kernel's static 2 KiB count against the default limit too)
        hipError_t e = hipFuncSetAttribute((const void*)tclu_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(tclu_means_kernel, dim3(r3d_cdiv(T, 4), B), dim3(256), 0, s, a);
    R3D_LAUNCH_CHECK();
    if (T > 1) {
        hipLaunchKernelGGL(tclu_pairs_kernel, dim3(tclu_nt(T), tclu_nt(T), B), dim3(256), lds, s, a);
        R3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tclu_finalize_kernel, dim3(1), dim3(256), 0, s, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_tcluster_bwd(const float* x, int ldx, int B, int T, int C, const int* starts, const int* last,
                                const int* count, const float* ws, const float* d_loss, float gscale, float* dx, int lddx,
                                int add, void* stream) {
    TcluArgs a = tclu_args(x, ldx, B, T, C, starts, last, count, const_cast<float*>(ws));
    a.d_loss = d_loss; a.gscale = gscale; a.dx = dx; a.lddx = lddx; a.add = add;
    int rc = tclu_check(a, true);
    if (rc != R3D_OK) return rc;
    hipLaunchKernelGGL(tclu_bwd_kernel, dim3(r3d_cdiv(T, 4), B), dim3(256), 0, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int64_t r3d_tcontrast_ws_floats(int B, int T) { return temporal_rows_ok(B, T) ? 5 * (int64_t)B * T : 0; }

static TconArgs tcon_args(const float* x, int ldx, int B, int T, int D, const int* first, const int* last, float temperature,
                          float* ws) {
    TconArgs a{};
    a.x = x; a.ld = ldx; a.B = B; a.T = T; a.D = D; a.first = first; a.last = last; a.ws = ws;
    a.inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    return a;
}

R3D_EXPORT int r3d_tcontrast_fwd(const float* x, int ldx, int B, int T, int D, const int* first, const int* last,
                                 float temperature, float* ws, float* loss_out, void* stream) {
    TconArgs a = tcon_args(x, ldx, B, T, D, first, last, temperature, ws);
    a.loss_out = loss_out;
    return tcon_dispatch(a, false, stream);
}

R3D_EXPORT int r3d_tcontrast_bwd(const float* x, int ldx, int B, int T, int D, const int* first, const int* last,
                                 float temperature, const float* ws, const float* d_loss, float gscale, float* dx, int lddx,
                                 int add, void* stream) {
    TconArgs a = tcon_args(x, ldx, B, T, D, first, last, temperature, const_cast<float*>(ws));
    a.d_loss = d_loss; a.gscale = gscale; a.dx = dx; a.lddx = lddx; a.add = add;
    return tcon_dispatch(a, true, stream);
}

R3D_EXPORT int r3d_focal_rows(const float* pred, int ld, const int64_t* gold, int N, int C, int64_t pad_idx, int has_exclude,
                              int64_t exclude_idx, float alpha, float gamma, float penalty_weight, float* ws, float* loss_out,
                              uint8_t* flags, int64_t* counts, const float* d_loss, float gscale, float* d_pred, int lddp,
                              int add, void* stream) {
    if (!pred || !gold || N < 1 || C < 1 || ld < C || !(gamma >= 1.0f)) return R3D_EINVAL;
    if (loss_out && (!ws || !flags || !counts)) return R3D_EINVAL;
    if (!loss_out && !d_pred) return R3D_EINVAL;
    if (d_pred && lddp < C) return R3D_EINVAL;
    FocalArgs a{};
    a.pred = pred; a.ld = ld; a.gold = gold; a.N = N; a.C = C; a.pad = pad_idx; a.excl = exclude_idx; a.has_excl = has_exclude;
    a.alpha = alpha; a.gamma = gamma; a.penalty = penalty_weight; a.ws = ws; a.loss_out = loss_out; a.flags = flags;
    a.counts = counts; a.d_loss = d_loss; a.gscale = gscale; a.dpred = d_pred; a.lddp = lddp; a.add = add;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(focal_rows_kernel, dim3(r3d_cdiv(N, 4)), dim3(256), 0, s, a);
    R3D_LAUNCH_CHECK();
    if (loss_out) {
        hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, s, a);
        R3D_LAUNCH_CHECK();
    }
    return R3D_OK;
}
