// On-device collate of a device-resident clip store (r3d_amd/clipcache.py): the padded batch that the reference's
// dataset + my_collate build on the host (data/basedataset_darai_depth.py:110-130,174-206: np.load -> observed slice ->
// sample rate -> torch.tensor -> pad_sequence) gathered from frame pools that already sit in HBM.
//
// One launch writes all five tensors of a batch.  Workgroups, in grid order:
//   * feature rows:  one per (destination row (b, s) of [B, S_f, D], chunk of 16 KiB of the row);
//   * depth rows:    one per (destination row of [B, S_d, P], 16-KiB chunk): a 224^2 frame is 13 chunks;
//   * label words:   one thread per element of past_label [B, S_l], trans_future_dur and trans_future_target [B, S_q].
// A destination row past its item's length is written with the padding value by the same workgroup (zero for frames,
// pad_idx for labels), so no memset precedes the launch.  Each lane keeps kUnroll dwordx4 loads in flight before it
// stores them (whole-row register gather: MI355X_MICROARCH.md "Indexed rows").  Rows whose length or base pointers are
// not 16-byte aligned take the dword path.  All row arithmetic is 64-bit: a pool of 10^6 224^2 frames is 5e10 floats.
#include "common.h"
#include "../../include/r3d_hip.h"

namespace r3d {

constexpr int kCollateThreads = 256;
constexpr int kUnroll = 4;                                    // dwordx4 per lane in flight
constexpr int64_t kChunkF4 = (int64_t)kCollateThreads * kUnroll;   // 1024 x 16 B = 16 KiB per workgroup
constexpr int64_t kChunkF = kChunkF4 * 4;                     // the same chunk in floats (dword path)
constexpr int64_t kMaxGrid = 1 << 20;                         // workgroups beyond this loop (grid-stride over chunks)

struct CollateGrid {
    int64_t cf, cd;                 // chunks per feature / depth row
    int64_t nf, nd, nl;             // workgroups of each part
    int32_t vec_f, vec_d;           // 16-byte path for the feature / depth rows
};

// Pool row of destination row s of item `item`, or -1 (padding): out-of-range items and pool ids read nothing.
__device__ __forceinline__ int64_t src_row(const int64_t* __restrict__ off, const int64_t* __restrict__ ids, int64_t n_items,
                                           int64_t n_pool, int64_t item, int64_t s) {
    if (item < 0 || item >= n_items) return -1;
    const int64_t o = off[item], n = off[item + 1] - o;
    if (s >= n) return -1;
    const int64_t r = ids[o + s];
    return (r >= 0 && r < n_pool) ? r : -1;
}

// Chunk `chunk` of one row of `len` floats: dst = src (or zeros when src == NULL).
__device__ __forceinline__ void copy_chunk(const float* __restrict__ src, float* __restrict__ dst, int64_t len, int64_t chunk,
                                           bool vec) {
    const int t = threadIdx.x;
    if (vec) {
        const int64_t n4 = len >> 2, base = chunk * kChunkF4;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        float4 v[kUnroll];
        if (src && base + kChunkF4 <= n4) {          // whole chunk in the row: no per-lane bounds, all loads before the stores
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) v[k] = s4[base + k * kCollateThreads + t];
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) d4[base + k * kCollateThreads + t] = v[k];
            return;
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const int64_t i = base + (int64_t)k * kCollateThreads + t;
            v[k] = (src && i < n4) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const int64_t i = base + (int64_t)k * kCollateThreads + t;
            if (i < n4) d4[i] = v[k];
        }
    } else {
        constexpr int kU = kUnroll * 4;
        const int64_t base = chunk * kChunkF;
        float v[kU];
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            const int64_t i = base + (int64_t)k * kCollateThreads + t;
            v[k] = (src && i < len) ? src[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            const int64_t i = base + (int64_t)k * kCollateThreads + t;
            if (i < len) dst[i] = v[k];
        }
    }
}

__global__ __launch_bounds__(kCollateThreads) void clip_collate_kernel(r3d_clip_collate_job j, CollateGrid g) {
    const int64_t total = g.nf + g.nd + g.nl;
    for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        if (blk < g.nf) {                                                         // feature rows
            const int64_t row = blk / g.cf, chunk = blk - row * g.cf;
            const int64_t b = row / j.S_f, s = row - b * j.S_f;
            const int64_t r = src_row(j.off_f, j.ids_f, j.n_items, j.F_rgb, j.items[b], s);
            copy_chunk(r >= 0 ? j.rgb_pool + r * j.D : nullptr, j.features + row * j.D, j.D, chunk, g.vec_f);
        } else if (blk < g.nf + g.nd) {                                           // depth rows
            const int64_t q = blk - g.nf;
            const int64_t row = q / g.cd, chunk = q - row * g.cd;
            const int64_t b = row / j.S_d, s = row - b * j.S_d;
            const int64_t r = src_row(j.off_d, j.ids_d, j.n_items, j.F_dep, j.items[b], s);
            copy_chunk(r >= 0 ? j.depth_pool + r * j.P : nullptr, j.depth + row * j.P, j.P, chunk, g.vec_d);
        } else {                                                                  // label words
            const int64_t e = (blk - g.nf - g.nd) * kCollateThreads + threadIdx.x;
            const int64_t nl = j.B * j.S_l, nq = j.B * j.S_q;
            if (e < nl) {
                const int64_t b = e / j.S_l, s = e - b * j.S_l, item = j.items[b];
                int64_t v = j.pad_idx;
                if (item >= 0 && item < j.n_items) {
                    const int64_t o = j.off_l[item];
                    if (s < j.off_l[item + 1] - o) v = j.lab[o + s];
                }
                j.past_label[e] = v;
            } else if (e < nl + nq) {
                const int64_t x = e - nl, b = x / j.S_q, s = x - b * j.S_q, item = j.items[b];
                float dur = (float)j.pad_idx;
                int64_t tgt = j.pad_idx;
                if (item >= 0 && item < j.n_items) {
                    const int64_t o = j.off_q[item];
                    if (s < j.off_q[item + 1] - o) {
                        dur = j.q_dur[o + s];
                        tgt = j.q_tgt[o + s];
                    }
                }
                j.trans_future_dur[x] = dur;
                j.trans_future_target[x] = tgt;
            }
        }
    }
}

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_clip_collate(const r3d_clip_collate_job* job, void* stream) {
    R3D_REQUIRE(job);
    const r3d_clip_collate_job& j = *job;
    R3D_REQUIRE(j.B >= 0 && j.n_items >= 0 && j.F_rgb >= 0 && j.F_dep >= 0 && j.D >= 0 && j.P >= 0);
    R3D_REQUIRE(j.S_f >= 0 && j.S_d >= 0 && j.S_l >= 0 && j.S_q >= 0);
    R3D_REQUIRE(j.F_rgb == 0 || (j.rgb_pool && j.D > 0));
    R3D_REQUIRE(j.F_dep == 0 || (j.depth_pool && j.P > 0));
    const bool any_f = j.B > 0 && j.S_f > 0 && j.D > 0, any_d = j.B > 0 && j.S_d > 0 && j.P > 0;
    const bool any_l = j.B > 0 && j.S_l > 0, any_q = j.B > 0 && j.S_q > 0;
    R3D_REQUIRE(!(any_f || any_d || any_l || any_q) || j.items);
    R3D_REQUIRE(!any_f || (j.features && j.off_f && (j.F_rgb == 0 || j.ids_f)));
    R3D_REQUIRE(!any_d || (j.depth && j.off_d && (j.F_dep == 0 || j.ids_d)));
    R3D_REQUIRE(!any_l || (j.past_label && j.off_l && j.lab));
    R3D_REQUIRE(!any_q || (j.trans_future_dur && j.trans_future_target && j.off_q && j.q_dur && j.q_tgt));
    CollateGrid g{};
    g.cf = any_f ? (j.D + kChunkF - 1) / kChunkF : 0;
    g.cd = any_d ? (j.P + kChunkF - 1) / kChunkF : 0;
    g.vec_f = (j.D % 4 == 0) && r3d_aligned16(j.rgb_pool) && r3d_aligned16(j.features);
    g.vec_d = (j.P % 4 == 0) && r3d_aligned16(j.depth_pool) && r3d_aligned16(j.depth);
    if (g.vec_f) g.cf = any_f ? ((j.D >> 2) + kChunkF4 - 1) / kChunkF4 : 0;
    if (g.vec_d) g.cd = any_d ? ((j.P >> 2) + kChunkF4 - 1) / kChunkF4 : 0;
    g.nf = any_f ? j.B * j.S_f * g.cf : 0;
    g.nd = any_d ? j.B * j.S_d * g.cd : 0;
    const int64_t words = (any_l ? j.B * j.S_l : 0) + (any_q ? j.B * j.S_q : 0);
    g.nl = (words + kCollateThreads - 1) / kCollateThreads;
    const int64_t total = g.nf + g.nd + g.nl;
    if (total == 0) return R3D_OK;
    hipLaunchKernelGGL(clip_collate_kernel, dim3((unsigned)(total < kMaxGrid ? total : kMaxGrid)), dim3(kCollateThreads), 0,
                       (hipStream_t)stream, j, g);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
