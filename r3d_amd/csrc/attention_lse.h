// What the two fp32 attention cores that keep lse and recompute the probabilities -- the tiled core (attention_tiled.hip)
// and the split-key core (attention_splitk.hip) -- share, so that they stay interchangeable on the same buffers: the
// argument block of every kernel of both, the key-mask predicate, the host check of an entry point's arguments and the
// function that fills the block from them.
#pragma once
#include "common.h"
#include "tile_mma.h"
#include "../../include/r3d_hip.h"

namespace r3d {

// The field order is the split-key kernels' (their instruction streams depend on it); the tiled kernels leave ws, chunk
// and nchunk unused.
struct LseArgs {
    const float *q, *k, *v;
    int ldq, ldk, ldv;
    const uint8_t* kpm;
    const int64_t* key_label;
    int pad_idx;
    const uint8_t* drop;
    float drop_scale;
    float* o;           // forward: written; backward: read
    int ldo;
    float* lse;         // [B][heads][Lq]
    const float* d_o;
    int lddo;
    float* delta;       // [B][heads][Lq]
    float *dq, *dk, *dv;
    int lddq, lddk, lddv;
    float* ws;          // split-key: the chunk partials
    int B, heads, Lq, Lk, dh;
    int chunk, nchunk;  // split-key: keys per workgroup, workgroups per (head, clip)
    float scale;        // 1 / sqrt(dh), set by lse_admit
};

__device__ __forceinline__ bool key_masked(const LseArgs& a, int b, int j) {
    if (j >= a.Lk) return true;
    const size_t e = (size_t)b * a.Lk + j;
    return (a.kpm && a.kpm[e]) || (a.key_label && a.key_label[e] == (int64_t)a.pad_idx);
}

// An entry point's parameters as the block; the forward entries pass nulls (and 0) for the backward's fields, the tiled
// entries a null ws.
static inline LseArgs lse_args(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint8_t* kpm,
                               const int64_t* key_label, int pad_idx, const uint8_t* drop, float drop_scale, const float* o,
                               int ldo, const float* lse, const float* d_o, int lddo, float* delta, float* dq, int lddq,
                               float* dk, int lddk, float* dv, int lddv, float* ws, int B, int heads, int Lq, int Lk, int dh) {
    LseArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.kpm = kpm;
    a.key_label = key_label; a.pad_idx = pad_idx; a.drop = drop; a.drop_scale = drop_scale;
    a.o = const_cast<float*>(o); a.ldo = ldo; a.lse = const_cast<float*>(lse); a.d_o = d_o; a.lddo = lddo; a.delta = delta;
    a.dq = dq; a.lddq = lddq; a.dk = dk; a.lddk = lddk; a.dv = dv; a.lddv = lddv; a.ws = ws;
    a.B = B; a.heads = heads; a.Lq = Lq; a.Lk = Lk; a.dh = dh;
    return a;
}

// The host check of both pairs (shape_ok: the core's own limits on Lq, Lk, dh; need_ws: the core writes a workspace),
// and after it the one place that sets scale: a refused dh never reaches the division.
static inline int lse_admit(LseArgs& a, bool shape_ok, bool bwd, bool need_ws) {
    if (!shape_ok) return R3D_EINVAL;
    if (!a.q || !a.k || !a.v || !a.o || !a.lse || (need_ws && !a.ws)) return R3D_EINVAL;
    if (a.B <= 0 || a.heads <= 0 || a.B > 65535 || a.heads > 65535) return R3D_EINVAL;
    const int H = a.heads * a.dh;
    if (a.ldq < H || a.ldk < H || a.ldv < H || a.ldo < H) return R3D_EINVAL;
    if (bwd && (!a.d_o || !a.delta || !a.dq || !a.dk || !a.dv || a.lddo < H || a.lddq < H || a.lddk < H || a.lddv < H))
        return R3D_EINVAL;
    a.scale = 1.0f / sqrtf((float)a.dh);
    return R3D_OK;
}

}  // namespace r3d
