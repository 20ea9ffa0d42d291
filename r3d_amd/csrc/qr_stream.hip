// Streaming QR for the effective rank of a whole data set: an upper-triangular R [H, H] with R^T R = sum X^T X over every
// row folded in so far, without ever forming the square (the Gram route squares the condition number: at one dominant
// direction with a 1e-4 tail the fp32 Gram error of the effective rank is ~1e-2, the Householder one ~1e-8).  R has the
// singular values of the whole [rows, H] matrix and goes to the Jacobi of erank.hip at the end.
//
//   r3d_qr_append: `lanes` independent accumulators R [lanes, H, H]; one workgroup per lane, lane g takes the contiguous
//     row slice [g ceil(n / lanes), ...) of X and walks it in tiles of T rows staged in LDS as [T][ld] (ld = H rounded
//     up to 4).  For column j = 0 .. H-1 one Householder reflector from R[j, j] and the tile's column j:
//         s = sum x^2, beta = -sign(R_jj) sqrt(R_jj^2 + s), v = x / (R_jj - beta), tau = (beta - R_jj) / beta
//     applied to row j of R and the tile's columns > j.  A tile column that is entirely zero takes no step (no 0/0), so
//     zero rows -- padded frames are staged as zeros -- provably change nothing.
//   r3d_qr_merge: lane g + stride folded into lane g for every pair at once: the same column loop with the other lane's
//     R rows as the appended rows (row i of an upper triangle is zero left of i: the loop of a tile starts at its first
//     row's column).  ceil(log2 lanes) launches leave the total in lane 0.
//
// Thread layout: G row groups x Hc columns (Hc = H rounded up to 64; H > 1024: two columns per thread).  Thread (g, c)
// owns column c of the tile rows t = g (mod G).  A column step is two barriers:
//   A  partial dots <x_j, x_c> over the thread's rows (x_j is one broadcast LDS address per row, x_c consecutive banks:
//      no bank conflicts) -> part[g][c];                                                                     barrier
//   B  every thread sums the G partials of its column and of column j (= s) in the order g = 0 .. G-1, forms beta / tau,
//      updates its rows of column c; row group 0 updates R[j, c] (read once, written once per tile, coalesced).  barrier
// `part` is double-buffered on the parity of j, so a skipped step (s == 0) needs no second barrier.  Every reduction has
// one fixed order, there are no atomics and no workgroup waits on another: the same (lanes, call sequence) gives the same bits.
// Range: s = sum x^2 is formed in fp32 without scaling, so a tile column whose squares all underflow (|x| below ~1e-23) counts
// as zero and is left out, and |x| above ~1e19 overflows s to inf.  LayerNorm / ReLU outputs are far inside; a caller with
// other data scales it first (the effective rank does not depend on a common factor).
#include "common.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int kQrMaxH = 2048;
constexpr int kQrMaxLanes = 64;
// dynamic LDS budget: the 256 B held back are required, not slack -- __syncthreads_or takes that much static LDS for its
// reduction, and at small H (T rows of 16 B) the tile fills the budget to the byte
constexpr int64_t kQrLds = 160 * 1024 - 256;

struct QrGeom { int Hc, cpt, G, ld, T; };

static inline bool qr_geom(int H, QrGeom* q) {
    if (H < 1 || H > kQrMaxH) return false;
    q->cpt = H > 1024 ? 2 : 1;
    q->Hc = q->cpt == 2 ? 1024 : (H + 63) / 64 * 64;
    q->G = q->Hc >= 512 ? 1 : 512 / q->Hc;                       // 512 threads up to H = 256, then one row group
    if (q->G > 8) q->G = 8;
    q->ld = (H + 3) & ~3;
    const int64_t vec = (int64_t)2 * q->G * q->Hc * q->cpt * 4;  // part[2][G][Hc * cpt]
    q->T = (int)((kQrLds - vec) / ((int64_t)q->ld * 4));
    return q->T >= 1;
}

struct QrArgs {
    const float* x;          // append: X [n, ldx]; merge: NULL (the source is lane g + stride of R)
    int64_t ldx;
    int n, per;              // append: rows, rows per lane
    const int64_t* row_label; int pad_idx;
    float* R;                // [lanes, H, H]
    int64_t* rows;           // [lanes] valid-row counters (NULL: not counted)
    int H, lanes, stride;    // stride > 0: merge
    QrGeom q;
};

template <int CPT>
__global__ __launch_bounds__(1024) void qr_fold_kernel(const QrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // part[2][G][Hc * CPT] | tile[T][ld]
    const int H = a.H, Hc = a.q.Hc, G = a.q.G, ld = a.q.ld, T = a.q.T;
    const int W = Hc * CPT;
    float* part = lds;
    float* tile = lds + 2 * G * W;
    const int tid = threadIdx.x, grp = tid / Hc, cl = tid - grp * Hc;
    const bool merge = a.stride > 0;
    int lane, r0, r1;
    const float* src;
    int64_t lds_src;
    if (merge) {
        lane = blockIdx.x * 2 * a.stride;
        if (lane + a.stride >= a.lanes) return;
        src = a.R + (int64_t)(lane + a.stride) * H * H;
        lds_src = H; r0 = 0; r1 = H;
    } else {
        lane = blockIdx.x;
        r0 = (int)min((int64_t)lane * a.per, (int64_t)a.n);
        r1 = (int)min((int64_t)r0 + a.per, (int64_t)a.n);
        if (r0 >= r1) return;
        src = a.x; lds_src = a.ldx;
    }
    float* R = a.R + (int64_t)lane * H * H;
    const int64_t* lab = merge ? nullptr : a.row_label;

    // ---- the lane's count of valid rows: wave 0, integer sums (exact in any order)
    if (a.rows != nullptr && tid < kWave) {
        long long cnt = 0;
        if (merge) {
            if (tid == 0) cnt = a.rows[lane + a.stride];
        } else {
            for (int r = r0 + tid; r < r1; r += kWave) cnt += (lab == nullptr || lab[r] != (int64_t)a.pad_idx) ? 1 : 0;
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, kWave);
        if (tid == 0) a.rows[lane] += cnt;
    }

    for (int t0 = r0; t0 < r1; t0 += T) {
        const int Tn = min(T, r1 - t0);
        // ---- stage the tile: thread (grp, cl) writes the rows it will own
        int any = 0;
        for (int t = grp; t < Tn; t += G) {
            const int r = t0 + t;
            const bool ok = lab == nullptr || lab[r] != (int64_t)a.pad_idx;
            any |= ok ? 1 : 0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int c = cl + k * Hc;
                if (c < H) tile[t * ld + c] = ok ? src[(int64_t)r * lds_src + c] : 0.0f;
            }
        }
        if (!__syncthreads_or(any)) continue;            // a tile of padding only: R stays as it is, bit for bit
        const int j0 = merge ? t0 : 0;                   // rows >= t0 of an upper triangle are zero left of column t0
        float rn[CPT], djn = 0.0f;                       // row j of R (this thread's columns) and R[j, j], one step ahead
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = cl + k * Hc;
            rn[k] = (c >= j0 && c < H) ? R[(int64_t)j0 * H + c] : 0.0f;
        }
        if (j0 < H) djn = R[(int64_t)j0 * H + j0];
        for (int j = j0; j < H; ++j) {
            float rc[CPT];
            const float alpha = djn;
#pragma unroll
            for (int k = 0; k < CPT; ++k) rc[k] = rn[k];
            if (j + 1 < H) {
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int c = cl + k * Hc;
                    rn[k] = (c > j && c < H) ? R[(int64_t)(j + 1) * H + c] : 0.0f;
                }
                djn = R[(int64_t)(j + 1) * H + j + 1];
            }
            float* pj = part + (j & 1) * G * W;
            // ---- A: partial dots of column j with this thread's columns over its rows
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int c = cl + k * Hc;
                if (c >= j && c < H) {
                    float d0 = 0.0f, d1 = 0.0f;
                    int t = grp;
                    for (; t + G < Tn; t += 2 * G) {
                        d0 = fmaf(tile[t * ld + j], tile[t * ld + c], d0);
                        d1 = fmaf(tile[(t + G) * ld + j], tile[(t + G) * ld + c], d1);
                    }
                    if (t < Tn) d0 = fmaf(tile[t * ld + j], tile[t * ld + c], d0);
                    pj[grp * W + c] = d0 + d1;
                }
            }
            __syncthreads();
            float s = 0.0f;
            for (int g = 0; g < G; ++g) s += pj[g * W + j];
            if (s == 0.0f) continue;                     // the tile's column j is all zero: no step (uniform over the block)
            // ---- B: the reflector, applied to row j of R and the thread's rows of its columns
            const float beta = alpha >= 0.0f ? -sqrtf(fmaf(alpha, alpha, s)) : sqrtf(fmaf(alpha, alpha, s));
            const float f = 1.0f / (alpha - beta);
            const float tau = (beta - alpha) / beta;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int c = cl + k * Hc;
                if (c > j && c < H) {
                    float dot = 0.0f;
                    for (int g = 0; g < G; ++g) dot += pj[g * W + c];
                    const float w = fmaf(dot, f, rc[k]);
                    const float coef = tau * w * f;
                    for (int t = grp; t < Tn; t += G) tile[t * ld + c] = fmaf(-coef, tile[t * ld + j], tile[t * ld + c]);
                    if (grp == 0) R[(int64_t)j * H + c] = fmaf(-tau, w, rc[k]);
                } else if (c == j && grp == 0) {
                    R[(int64_t)j * H + j] = beta;
                }
            }
            __syncthreads();
        }
        __syncthreads();                                 // the tile is dead: the next one may be staged over it
    }
}

static int qr_launch(const QrArgs& a, int grid, hipStream_t st) {
    const QrGeom& q = a.q;
    const int64_t lds = ((int64_t)2 * q.G * q.Hc * q.cpt + (int64_t)q.T * q.ld) * 4;
    const int threads = q.G * q.Hc;
    if (q.cpt == 2) {
        hipError_t e = hipFuncSetAttribute((const void*)qr_fold_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(qr_fold_kernel<2>, dim3(grid), dim3(threads), (size_t)lds, st, a);
    } else {
        hipError_t e = hipFuncSetAttribute((const void*)qr_fold_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(qr_fold_kernel<1>, dim3(grid), dim3(threads), (size_t)lds, st, a);
    }
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_qr_append_supported(int H) {
    QrGeom q;
    return qr_geom(H, &q) ? 1 : 0;
}

R3D_EXPORT int r3d_qr_append_tile_rows(int H) {
    QrGeom q;
    return qr_geom(H, &q) ? q.T : 0;
}

R3D_EXPORT int r3d_qr_append(const float* x, int64_t ldx, int n, int H, const int64_t* row_label, int pad_idx, float* R,
                             int64_t* rows, int lanes, void* stream) {
    QrArgs a;
    R3D_REQUIRE(qr_geom(H, &a.q));
    R3D_REQUIRE(lanes >= 1 && lanes <= kQrMaxLanes && n >= 0 && ldx >= H && R != nullptr);
    if (n == 0) return R3D_OK;
    R3D_REQUIRE(x != nullptr);
    a.x = x; a.ldx = ldx; a.n = n; a.per = (n + lanes - 1) / lanes;
    a.row_label = row_label; a.pad_idx = pad_idx; a.R = R; a.rows = rows; a.H = H; a.lanes = lanes; a.stride = 0;
    return qr_launch(a, lanes, (hipStream_t)stream);
}

R3D_EXPORT int r3d_qr_merge(float* R, int64_t* rows, int H, int lanes, int stride, void* stream) {
    QrArgs a;
    R3D_REQUIRE(qr_geom(H, &a.q));
    R3D_REQUIRE(lanes >= 1 && lanes <= kQrMaxLanes && stride >= 1 && R != nullptr);
    if (stride >= lanes) return R3D_OK;
    a.x = nullptr; a.ldx = H; a.n = H; a.per = H; a.row_label = nullptr; a.pad_idx = 0;
    a.R = R; a.rows = rows; a.H = H; a.lanes = lanes; a.stride = stride;
    return qr_launch(a, (lanes + 2 * stride - 1) / (2 * stride), (hipStream_t)stream);
}
