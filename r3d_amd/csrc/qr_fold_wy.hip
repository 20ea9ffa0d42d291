// Blocked fold of rows into the streaming-QR accumulators of qr_stream.hip: the tile-QR "TS" step on [R; tile] in the
// compact-WY form, so that everything right of a 16-column panel is updated by fp32-input MFMA products instead of one
// reflector at a time.  Same contract as r3d_qr_append without labels: `lanes` accumulators R [lanes, H, H], one workgroup
// per lane, lane g takes rows [g ceil(n / lanes), ...); the result is upper-triangular with R^T R = sum X^T X (diagonal
// signs free) and goes to the unchanged r3d_qr_merge.
//
// Per tile of T rows (LDS [T][ld], rows past the slice zero) and per panel j0 .. j0 + 15:
//   1  the panel's 16 tile columns are copied to VQ [T][16], rows j0 .. j0 + 15 of R (columns >= j0) to RP [16][ld];
//   2  the panel is factored with the reflector formula of qr_stream.hip on its own 16 columns only: reflector jj is
//      [e_jj ; v_jj] (R is upper-triangular: it touches row jj of R and the tile), v = x / (R_jj - beta),
//      tau = (beta - R_jj) / beta.  512 threads = 16 columns x 32 row groups, two barriers per column.  A panel column
//      that is entirely zero takes tau = 0, v = 0 (no 0/0: zero rows change nothing);
//   3  V = the scaled columns, kept twice: VQ (row stride 16, k-major MFMA operand) and VP (row stride 18, row-major operand);
//   4  S = V^T V (one wave, MFMA), then T [16, 16] upper-triangular with H_0 .. H_15 = I - Y T Y^T, Y = [I; V]:
//      T_jj = tau_j, T[0:j, j] = -tau_j T[0:j, 0:j] S[0:j, j]; row i of T only needs its own earlier entries: one thread each;
//   5  for every 16-column block c right of the panel (one wave each, 8 at a time):
//          Z = R[panel, c] + V^T A[:, c]     (MFMA over the tile's rows)
//          W = T^T Z                          (MFMA, Z through LDS into the operand layout)
//          R[panel, c] -= W,   A[:, c] -= V W (MFMA per 16 rows of the tile)
//   6  RP goes back to R (on and right of the diagonal only: what lies below is never read or written).
// Every sum has one fixed order (the MFMA's k order, the row-group order g = 0 .. 31), there are no atomics and no workgroup
// waits on another: the same (lanes, call) gives the same bits.  Range: as qr_stream.hip (sum x^2 in fp32, unscaled).
//
// LDS banking (ds_read_b32 / ds_write_b32: 32 banks, per 32-lane half = two MFMA k-rows of 16 lanes): ld = 16 (mod 32) makes
// the k-major reads of the tile conflict-free (the 4-row read-modify-write of step 5 is 2-way); VQ's stride 16 the same;
// VP's stride 18 gives 16 rows x 2 k 32 distinct banks; the small matrices use stride 20 (rows 4 apart: 16 banks apart).
#include "common.h"
#include "tile_mma.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int kWyNb = 16;                 // panel width = MFMA tile
constexpr int kWyThreads = 512, kWyWaves = 8, kWyNG = kWyThreads / kWyNb;
constexpr int kWyVP = 18, kWySm = 20;
constexpr int kWyMaxLanes = 64, kWyMaxH = 2048;
constexpr int kWyMinT = 32, kWyMaxT = 512;
constexpr int64_t kWyLds = 160 * 1024 - 256;

struct WyGeom { int ld, T; int64_t floats; };

static inline int64_t wy_fixed_floats(int ld) {
    return (int64_t)kWyNb * ld + 2 * kWyNG * kWyNb + 2 * kWyNb * kWySm + kWyWaves * kWyNb * kWySm + 2 * kWyNb;
}

// admitted: H a multiple of 16 whose tile has at least kWyMinT rows next to the 16 staged rows of R -- 16 .. 720 today
static inline bool wy_geom(int H, WyGeom* q) {
    if (H < kWyNb || H > kWyMaxH || H % kWyNb != 0) return false;
    q->ld = (H % 32 == 16) ? H : H + 16;
    const int64_t per_row = q->ld + kWyNb + kWyVP;
    int64_t T = (kWyLds / 4 - wy_fixed_floats(q->ld)) / per_row;
    T = T / 16 * 16;
    if (T > kWyMaxT) T = kWyMaxT;
    if (T < kWyMinT) return false;
    q->T = (int)T;
    q->floats = T * per_row + wy_fixed_floats(q->ld);
    return true;
}

struct WyArgs {
    const float* x;
    int64_t ldx;
    int n, per;
    float* R;
    int H, lanes;
    WyGeom q;
};

__device__ __forceinline__ f32x4 wy_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(kWyThreads) void qr_fold_wy_kernel(const WyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, ld = a.q.ld, T = a.q.T;
    float* tile = lds;                               // [T][ld]
    float* VQ = tile + (size_t)T * ld;               // [T][16]
    float* VP = VQ + (size_t)T * kWyNb;              // [T][18]
    float* RP = VP + (size_t)T * kWyVP;              // [16][ld]
    float* part = RP + kWyNb * ld;                   // [2][32][16]
    float* Sm = part + 2 * kWyNG * kWyNb;            // [16][20]
    float* TM = Sm + kWyNb * kWySm;                  // [16][20]
    float* ZS = TM + kWyNb * kWySm;                  // [8][16][20]
    float* tau = ZS + kWyWaves * kWyNb * kWySm;      // [16]
    float* fs = tau + kWyNb;                         // [16]
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, c = l & 15, kq = l >> 4;
    const int pc = tid & 15, pg = tid >> 4;          // panel factorisation: column, row group
    float* zs = ZS + wave * kWyNb * kWySm;

    const int lane = blockIdx.x;
    const int r0 = (int)min((int64_t)lane * a.per, (int64_t)a.n);
    const int r1 = (int)min((int64_t)r0 + a.per, (int64_t)a.n);
    if (r0 >= r1) return;
    float* R = a.R + (int64_t)lane * H * H;

    for (int t0 = r0; t0 < r1; t0 += T) {
        const int Tn = min(T, r1 - t0), Tp = (Tn + 15) & ~15;
        for (int e = tid; e < Tp * H; e += kWyThreads) {
            const int t = e / H, cc = e - t * H;
            tile[t * ld + cc] = t < Tn ? a.x[(int64_t)(t0 + t) * a.ldx + cc] : 0.0f;
        }
        __syncthreads();
        for (int j0 = 0; j0 < H; j0 += kWyNb) {
            const int Wd = H - j0;                   // columns of R's rows from the panel on
            // ---- 1: the panel's columns and R's rows
            for (int e = tid; e < Tp * kWyNb; e += kWyThreads) VQ[e] = tile[(e >> 4) * ld + j0 + (e & 15)];
            for (int e = tid; e < kWyNb * Wd; e += kWyThreads) {
                const int i = e / Wd, cc = e - i * Wd;
                RP[i * ld + j0 + cc] = cc >= i ? R[(int64_t)(j0 + i) * H + j0 + cc] : 0.0f;
            }
            __syncthreads();
            // ---- 2: the panel's 16 reflectors
            for (int jj = 0; jj < kWyNb; ++jj) {
                float* pj = part + (jj & 1) * kWyNG * kWyNb;
                const float alpha = RP[jj * ld + j0 + jj], rc = RP[jj * ld + j0 + pc];     // (row jj is written at step jj only)
                if (pc >= jj) {
                    float d = 0.0f;
                    for (int t = pg; t < Tp; t += kWyNG) d = fmaf(VQ[t * kWyNb + jj], VQ[t * kWyNb + pc], d);
                    pj[pg * kWyNb + pc] = d;
                }
                __syncthreads();
                float s = 0.0f;
                for (int g = 0; g < kWyNG; ++g) s += pj[g * kWyNb + jj];
                if (s == 0.0f) {                     // the tile's column is all zero: the identity (uniform over the block)
                    if (tid == 0) { tau[jj] = 0.0f; fs[jj] = 0.0f; }
                    continue;
                }
                const float beta = alpha >= 0.0f ? -sqrtf(fmaf(alpha, alpha, s)) : sqrtf(fmaf(alpha, alpha, s));
                const float f = 1.0f / (alpha - beta);
                const float tv = (beta - alpha) / beta;
                if (pc > jj) {
                    float dot = 0.0f;
                    for (int g = 0; g < kWyNG; ++g) dot += pj[g * kWyNb + pc];
                    const float w = fmaf(dot, f, rc);
                    const float coef = tv * w * f;
                    for (int t = pg; t < Tp; t += kWyNG) VQ[t * kWyNb + pc] = fmaf(-coef, VQ[t * kWyNb + jj], VQ[t * kWyNb + pc]);
                    if (pg == 0) RP[jj * ld + j0 + pc] = fmaf(-tv, w, rc);
                } else if (pc == jj && pg == 0) {
                    RP[jj * ld + j0 + jj] = beta;
                    tau[jj] = tv;
                    fs[jj] = f;
                }
                __syncthreads();
            }
            __syncthreads();                         // (a skipped last step leaves tau / fs without a barrier behind them)
            if (Wd > kWyNb) {
                // ---- 3: V = x f, in both operand layouts
                {
                    const float f = fs[pc];
                    for (int t = pg; t < Tp; t += kWyNG) {
                        const float v = VQ[t * kWyNb + pc] * f;
                        VQ[t * kWyNb + pc] = v;
                        VP[t * kWyVP + pc] = v;
                    }
                }
                __syncthreads();
                // ---- 4: S = V^T V, then T
                if (wave == 0) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    for (int k0 = 0; k0 < Tp; k0 += 4) {
                        const float v = VQ[(k0 + kq) * kWyNb + c];
                        acc = wy_mfma(v, v, acc);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) Sm[(4 * kq + i) * kWySm + c] = acc[i];
                }
                __syncthreads();
                if (tid < kWyNb) {
                    float trow[kWyNb];
#pragma unroll
                    for (int j = 0; j < kWyNb; ++j) {
                        float acc = 0.0f;
#pragma unroll
                        for (int k = 0; k < j; ++k) acc = fmaf(trow[k], Sm[k * kWySm + j], acc);
                        trow[j] = j == tid ? tau[j] : (j > tid ? -tau[j] * acc : 0.0f);
                        TM[tid * kWySm + j] = trow[j];
                    }
                }
                __syncthreads();
                // ---- 5: everything right of the panel, 16 columns per wave
                const int nblk = (Wd - kWyNb) / kWyNb;
                for (int rd = 0; rd * kWyWaves < nblk; ++rd) {
                    const int cb = rd * kWyWaves + wave;
                    const bool active = cb < nblk;
                    const int c0 = j0 + kWyNb + cb * kWyNb;
                    if (active) {
                        f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        for (int k0 = 0; k0 < Tp; k0 += 4) z = wy_mfma(VQ[(k0 + kq) * kWyNb + c], tile[(k0 + kq) * ld + c0 + c], z);
#pragma unroll
                        for (int i = 0; i < 4; ++i) zs[(4 * kq + i) * kWySm + c] = z[i] + RP[(4 * kq + i) * ld + c0 + c];
                    }
                    __syncthreads();
                    f32x4 w = {0.f, 0.f, 0.f, 0.f};
                    if (active) {
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) w = wy_mfma(TM[(4 * ks + kq) * kWySm + c], zs[(4 * ks + kq) * kWySm + c], w);
#pragma unroll
                        for (int i = 0; i < 4; ++i) RP[(4 * kq + i) * ld + c0 + c] -= w[i];
                    }
                    __syncthreads();
                    if (active) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) zs[(4 * kq + i) * kWySm + c] = w[i];
                    }
                    __syncthreads();
                    if (active) {
                        float wb[4];
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) wb[ks] = zs[(4 * ks + kq) * kWySm + c];
                        for (int tb = 0; tb < Tp; tb += 16) {
                            f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int ks = 0; ks < 4; ++ks) u = wy_mfma(VP[(tb + c) * kWyVP + 4 * ks + kq], wb[ks], u);
#pragma unroll
                            for (int i = 0; i < 4; ++i) tile[(tb + 4 * kq + i) * ld + c0 + c] -= u[i];
                        }
                    }
                    __syncthreads();                 // (zs is written again by the next round)
                }
            }
            // ---- 6: R's rows go back
            for (int e = tid; e < kWyNb * Wd; e += kWyThreads) {
                const int i = e / Wd, cc = e - i * Wd;
                if (cc >= i) R[(int64_t)(j0 + i) * H + j0 + cc] = RP[i * ld + j0 + cc];
            }
            __syncthreads();
        }
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_qr_fold_wy_supported(int H) {
    WyGeom q;
    return wy_geom(H, &q) ? 1 : 0;
}

R3D_EXPORT int r3d_qr_fold_wy_tile_rows(int H) {
    WyGeom q;
    return wy_geom(H, &q) ? q.T : 0;
}

R3D_EXPORT int r3d_qr_fold_wy(const float* x, int64_t ldx, int n, int H, float* R, int lanes, void* stream) {
    WyArgs a;
    R3D_REQUIRE(wy_geom(H, &a.q));
    R3D_REQUIRE(lanes >= 1 && lanes <= kWyMaxLanes && n >= 0 && ldx >= H && R != nullptr);
    if (n == 0) return R3D_OK;
    R3D_REQUIRE(x != nullptr);
    a.x = x; a.ldx = ldx; a.n = n; a.per = (n + lanes - 1) / lanes; a.R = R; a.H = H; a.lanes = lanes;
    const int64_t bytes = a.q.floats * 4;
    hipError_t e = hipFuncSetAttribute((const void*)qr_fold_wy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(qr_fold_wy_kernel, dim3(lanes), dim3(kWyThreads), (size_t)bytes, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
