// On-device collate of a device-resident clip store (r3d_amd/clipcache.py): the padded batch that the reference's
// dataset + my_collate build on the host (data/basedataset_darai_depth.py:110-130,174-206: np.load -> observed slice ->
// sample rate -> torch.tensor -> pad_sequence) gathered from frame pools that already sit in HBM.
//
// Two entry points: r3d_clip_collate for the five tensors of the depth dataset (below), and r3d_clip_collate_tracks for a
// batch described as a list of tracks (further down).
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

// Chunk `chunk` of one row of `len` floats: dst = src (or `pad` when src == NULL).
__device__ __forceinline__ void copy_chunk(const float* __restrict__ src, float* __restrict__ dst, int64_t len, int64_t chunk,
                                           bool vec, float pad = 0.f) {
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
            v[k] = (src && i < n4) ? s4[i] : make_float4(pad, pad, pad, pad);
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
            v[k] = (src && i < len) ? src[i] : pad;
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

// ---- the same launch over a list of tracks (r3d_clip_collate_tracks) ---------------------------------------------------
// Frame rows of R3D_CLIP_WIDE_ROW floats or more keep the mapping above.  Narrower rows (a gaze row is 2 to 8 floats) and
// the word tracks are PACKED: a workgroup writes kPackElems consecutive elements of the track's output in kPackRounds
// rounds; in a round each lane takes kPackU elements a workgroup's width apart, so every store instruction of a wave covers
// 64 consecutive elements whatever the row length, and a track of 8-byte rows costs one workgroup per 16 KiB instead of one
// per row.  An element finds its row from its index (row = e / width, column = e % width); its chain of dependent loads
// (items -> off -> ids -> pool) is one of kPackU independent chains a lane has in flight before the round's stores.
constexpr int kPackU = 4;
constexpr int kPackRounds = 4;                  // (rounds are not unrolled: each element costs two 64-bit divisions of code)
constexpr int64_t kPackElems = (int64_t)kCollateThreads * kPackU * kPackRounds;   // 4096 elements: 16 KiB of fp32

//
// Grid order: the packed tracks' workgroups come FIRST, then the wide rows.  A packed workgroup is a few microseconds of
// dependent-load latency and almost no bytes; at the head of the grid it runs under the wide rows' traffic, at the tail it
// would be the launch's last workgroup (measured, tools/clip_tracks_speed.py).  The outputs' order is the tracks' order
// either way.  A workgroup finds its segment without a dependent load: the segment starts are compared as constants of the
// launch, and the segment's track is a nibble of `order`.
struct TracksGrid {
    int64_t start[R3D_CLIP_MAX_TRACKS];         // first workgroup of each grid segment (segments past the last: INT64_MAX)
    int64_t total;                              // all workgroups
    uint32_t order;                             // nibble s: the track of grid segment s
    int64_t chunks[R3D_CLIP_MAX_TRACKS];        // by track; wide rows: 16-KiB chunks per row; 0: the packed path
    int32_t vec[R3D_CLIP_MAX_TRACKS];           // by track; wide rows: the 16-byte path
};

// Workgroup q of a packed track.  kFrames: T = float rows gathered through ids; otherwise words of T, row = element.
template <typename T, bool kFrames>
__device__ __forceinline__ void pack_elements(const int64_t* __restrict__ items, int64_t n_items, int64_t B,
                                              const r3d_clip_track& k, int64_t q) {
    const T* __restrict__ src = static_cast<const T*>(k.src);
    T* __restrict__ out = static_cast<T*>(k.out);
    const int64_t width = kFrames ? k.width : 1, n = B * k.S * width;
    const T pad = (T)k.pad;
#pragma unroll 1
    for (int g = 0; g < kPackRounds; ++g) {
        const int64_t e0 = q * kPackElems + (int64_t)g * kPackU * kCollateThreads + threadIdx.x;
        if (e0 - threadIdx.x >= n) break;
        T v[kPackU];
#pragma unroll
        for (int u = 0; u < kPackU; ++u) {
            const int64_t e = e0 + (int64_t)u * kCollateThreads;
            v[u] = pad;
            if (e < n) {
                const int64_t row = kFrames ? e / width : e, col = e - row * width;
                const int64_t b = row / k.S, s = row - b * k.S, item = items[b];
                if (item >= 0 && item < n_items) {
                    const int64_t o = k.off[item];
                    if (s < k.off[item + 1] - o) {
                        const int64_t r = kFrames ? k.ids[o + s] : o + s;
                        if (r >= 0 && r < k.rows) v[u] = src[r * width + col];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kPackU; ++u) {
            const int64_t e = e0 + (int64_t)u * kCollateThreads;
            if (e < n) out[e] = v[u];
        }
    }
}

__global__ __launch_bounds__(kCollateThreads) void clip_collate_tracks_kernel(r3d_clip_tracks_job j, TracksGrid g) {
    for (int64_t blk = blockIdx.x; blk < g.total; blk += gridDim.x) {
        int seg = 0;
        int64_t first = 0;                                  // (start[0] = 0; the starts ascend, so the last one reached wins)
#pragma unroll
        for (int i = 1; i < R3D_CLIP_MAX_TRACKS; ++i) {
            if (blk >= g.start[i]) {
                seg = i;
                first = g.start[i];
            }
        }
        const int t = (g.order >> (4 * seg)) & 15;
        const r3d_clip_track& k = j.tracks[t];
        const int64_t q = blk - first;
        if (g.chunks[t] > 0) {                                                    // wide frame rows
            const int64_t row = q / g.chunks[t], chunk = q - row * g.chunks[t];
            const int64_t b = row / k.S, s = row - b * k.S;
            const int64_t r = src_row(k.off, k.ids, j.n_items, k.rows, j.items[b], s);
            copy_chunk(r >= 0 ? static_cast<const float*>(k.src) + r * k.width : nullptr,
                       static_cast<float*>(k.out) + row * k.width, k.width, chunk, g.vec[t], (float)k.pad);
        } else if (k.kind == R3D_CLIP_FRAMES_F32) {
            pack_elements<float, true>(j.items, j.n_items, j.B, k, q);
        } else if (k.kind == R3D_CLIP_WORDS_I64) {
            pack_elements<int64_t, false>(j.items, j.n_items, j.B, k, q);
        } else {
            pack_elements<float, false>(j.items, j.n_items, j.B, k, q);
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

R3D_EXPORT int r3d_clip_collate_tracks(const r3d_clip_tracks_job* job, void* stream) {
    R3D_REQUIRE(job);
    const r3d_clip_tracks_job& j = *job;
    R3D_REQUIRE(j.n_tracks >= 0 && j.n_tracks <= R3D_CLIP_MAX_TRACKS && j.B >= 0 && j.n_items >= 0);
    TracksGrid g{};
    int64_t count[R3D_CLIP_MAX_TRACKS] = {};                    // workgroups of each track
    for (int t = 0; t < j.n_tracks; ++t) {
        const r3d_clip_track& k = j.tracks[t];
        const bool frames = k.kind == R3D_CLIP_FRAMES_F32;
        R3D_REQUIRE(frames || k.kind == R3D_CLIP_WORDS_I64 || k.kind == R3D_CLIP_WORDS_F32);
        R3D_REQUIRE(k.S >= 0 && k.rows >= 0);
        int64_t& n = count[t];
        if (j.B > 0 && k.S > 0) {
            R3D_REQUIRE(frames ? k.width > 0 : k.width == 1);
            R3D_REQUIRE(j.items && k.off && k.out);
            R3D_REQUIRE(k.rows == 0 || (k.src && (!frames || k.ids)));
            if (frames && k.width >= R3D_CLIP_WIDE_ROW) {
                g.vec[t] = (k.width % 4 == 0) && r3d_aligned16(k.src) && r3d_aligned16(k.out);
                g.chunks[t] = g.vec[t] ? ((k.width >> 2) + kChunkF4 - 1) / kChunkF4 : (k.width + kChunkF - 1) / kChunkF;
                n = j.B * k.S * g.chunks[t];
            } else {
                n = (j.B * k.S * k.width + kPackElems - 1) / kPackElems;
            }
        }
    }
    int seg = 0;                                                // grid segments: the packed tracks, then the wide ones
    for (int wide = 0; wide < 2; ++wide) {
        for (int t = 0; t < j.n_tracks; ++t) {
            if (count[t] == 0 || (g.chunks[t] > 0) != (wide == 1)) continue;
            g.start[seg] = g.total;
            g.order |= (uint32_t)t << (4 * seg);
            g.total += count[t];
            ++seg;
        }
    }
    for (; seg < R3D_CLIP_MAX_TRACKS; ++seg) g.start[seg] = INT64_MAX;
    if (g.total == 0) return R3D_OK;
    hipLaunchKernelGGL(clip_collate_tracks_kernel, dim3((unsigned)(g.total < kMaxGrid ? g.total : kMaxGrid)),
                       dim3(kCollateThreads), 0, (hipStream_t)stream, j, g);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
