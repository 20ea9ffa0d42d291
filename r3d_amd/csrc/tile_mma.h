// The 64 x 64 tile discipline shared by the tiled and split-key attention cores (attention_tiled.hip,
// attention_splitk.hip), the contrastive losses (supcon.hip, temporal.hip) and the CNN's head (cnn.hip): 256 threads = 4 waves, operand tiles of 64 rows staged in LDS with the width zero-padded to DP and
// a row stride of DP + 4 floats, score tiles of 64 x 64 with a row stride of 68.  Wave w owns rows [16w, 16w + 16) of
// a tile; every product is a chain of fp32-input 16x16x4 MFMAs on LDS operands (exact fp32, one VGPR per operand).
// Each lane feeds FOUR k-steps from one 16-byte LDS read: step t of lane (c, kq) carries k = k0 + 4 kq + t on both
// operands, a permutation of the k order inside a 16-wide group that A and B share.
#pragma once
#include "common.h"

namespace r3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TT = 64;          // tile rows (queries) and columns (keys)
constexpr int SLD = TT + 4;     // score tile row stride: 16 rows x 4 lanes of a wave hit 64 distinct banks

__device__ __forceinline__ float4 lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// rows [row0, row0 + 64) x [0, dh) of a strided matrix -> LDS [64][DP + 4]; rows past L and columns past dh are zero.
// 16-byte loads where the head's rows allow them (the engine's slices do), single floats otherwise (dh 5, odd offsets).
// (ROWS: the split-key core, attention_splitk.hip, stages its 16 query rows with the same code.)
template <int DP, int ROWS = TT>
__device__ __forceinline__ void stage_tile(float* dst, const float* base, int ld, int row0, int L, int dh, int tid) {
    constexpr int LD = DP + 4;
    if (((reinterpret_cast<uintptr_t>(base) & 15u) | (ld & 3) | (dh & 3)) == 0) {
        for (int e = tid; e < ROWS * DP / 4; e += 256) {
            const int r = e / (DP / 4), d = (e % (DP / 4)) * 4;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < L && d < dh) x = *reinterpret_cast<const float4*>(base + (size_t)(row0 + r) * ld + d);
            *reinterpret_cast<float4*>(dst + r * LD + d) = x;
        }
        return;
    }
    for (int e = tid; e < ROWS * DP; e += 256) {
        const int r = e / DP, d = e % DP;
        float x = 0.f;
        if (row0 + r < L && d < dh) x = base[(size_t)(row0 + r) * ld + d];
        dst[r * LD + d] = x;
    }
}

// acc[16 x 16] += A[16 rows][DP] . B[16 rows][DP]^T, both LDS row-major with stride DP + 4: row of acc <- row of A, column <- row of B
template <int DP>
__device__ __forceinline__ void mma_nt(f32x4& acc, const float* A, const float* Bm, int c, int kq) {
    constexpr int LD = DP + 4;
    const float* ap = A + c * LD + 4 * kq;
    const float* bp = Bm + c * LD + 4 * kq;
#pragma unroll
    for (int k0 = 0; k0 < DP; k0 += 16) {
        const float4 a = lds4(ap + k0), b = lds4(bp + k0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
}

// acc[n] (16 x 16, columns [16n, 16n + 16)) += P[16 rows][64] . M[64 rows][DP]: P with stride SLD, M with stride DP + 4
template <int DP>
__device__ __forceinline__ void mma_nn(f32x4 (&acc)[DP / 16], const float* P, const float* M, int c, int kq) {
    constexpr int LD = DP + 4;
#pragma unroll
    for (int j0 = 0; j0 < TT; j0 += 16) {
        const float4 a = lds4(P + c * SLD + j0 + 4 * kq);
        const float* mp = M + (j0 + 4 * kq) * LD + c;
#pragma unroll
        for (int n = 0; n < DP / 16; ++n) {
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, mp[16 * n], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, mp[LD + 16 * n], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, mp[2 * LD + 16 * n], acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, mp[3 * LD + 16 * n], acc[n], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ float quad_sum(float v) {       // over the 4 lanes of a row, fixed order
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}

// ---- host side of every user ------------------------------------------------------------------------------------------
// the padded width DP of the instance that runs a head / row width (each user's own check caps the width)
static inline int tile_dp(int width) { return width <= 16 ? 16 : width <= 32 ? 32 : width <= 64 ? 64 : width <= 128 ? 128 : 256; }

// a kernel launched with more than 64 KiB of dynamic LDS has to opt in (per device, so at every call); the HIP error
static inline hipError_t allow_dynamic_lds(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace r3d
