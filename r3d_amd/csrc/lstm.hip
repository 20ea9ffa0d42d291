// The recurrence of a bidirectional nn.LSTM layer (batch_first, h0 = c0 = 0, gate order i, f, g, o), forward and backward,
// for the RNN baseline of the reference (model/rnn.py:20,93: nn.LSTM(H, H/2, num_layers=2, bidirectional=True)).
//
// What is NOT here: the input projection G_in = X W_ih^T + b_ih of both directions is one GEMM before the forward launch,
// and dW_ih, dW_hh, the bias gradients and dX are GEMMs after the backward launch (the existing r3d_gemm_f32 family).
//
// One workgroup per (clip, direction): grid = 2 B, workgroup = 4h threads rounded up to a whole wave.  Thread j < 4h owns
// one gate row and holds its h weights of W_hh in registers for the whole walk (at h = 128 that is 128 VGPRs a lane, two
// waves per SIMD); the running state lives in LDS.  Per step the forward is
//     gates_j = G_in[t, j] + b_hh[j] + W_hh[j, :] . h_{t-1}      (h_{t-1} read from LDS as a broadcast, fp32 FMAs)
//     i, f, o = sigmoid, g = tanh;  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
// with two barriers; it stores the activated gates, c_t and h_{t-1} (time-aligned, so that dW_hh = dG^T H_prev is a plain
// TN product).  The backward walks the same steps in reverse order; thread (q, m) holds the column m of the gate block q
// of W_hh, so dh_{t-1} = sum_q (dG_q . W_hh[q-block, m]) is four register dot products added in a fixed order.  No
// atomics and no cross-workgroup traffic: results are bitwise reproducible.
#include "common.h"
#include "../../include/r3d_hip.h"

namespace r3d {

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct LstmFwdArgs {
    const float* gin; int ldgin;           // [B*S, 8h]: X W_ih^T + b_ih, direction d at columns [4h d, 4h d + 4h)
    const float* whh0; const float* whh1;  // [4h, h] per direction
    const float* bhh0; const float* bhh1;  // [4h]
    float* y; int ldy;                     // [B*S, 2h]: h_t, direction d at columns [h d, h d + h)
    float* gates; int ldgates;             // [B*S, 8h]: activated gates
    float* cell; int ldcell;               // [B*S, 2h]: c_t
    float* hprev; int ldhprev;             // [B*S, 2h]: h_{t-1} in the direction's own order (0 at its first step)
    int B, S, h;
};

struct LstmBwdArgs {
    const float* dy; int lddy;             // [B*S, 2h]: dL/dh_t from above (the layer's output gradient)
    const float* whh0; const float* whh1;
    const float* gates; int ldgates;
    const float* cell; int ldcell;
    float* dg; int lddg;                   // [B*S, 8h]: dL/d(pre-activation gates)
    int B, S, h;
};

template <int HM>
__global__ __launch_bounds__(512) void lstm_fwd_kernel(const LstmFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float hs[HM];
    __shared__ float gs[4 * HM];
    const int h = a.h, G = 4 * h, S = a.S;
    const int b = (int)blockIdx.x >> 1, d = (int)blockIdx.x & 1;
    const int tid = (int)threadIdx.x;
    const bool act = tid < G;
    const float* W = d ? a.whh1 : a.whh0;
    const float bias = act ? (d ? a.bhh1 : a.bhh0)[tid] : 0.f;
    float w[HM];
#pragma unroll
    for (int k = 0; k < HM; k += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[k + e] = 0.f;
        if (act && k < h) {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[k + e] = W[(size_t)tid * h + k + e];
        }
    }
    for (int k = tid; k < h; k += (int)blockDim.x) hs[k] = 0.f;
    __syncthreads();
    const int q = act ? tid / h : 0;
    const size_t row0 = (size_t)b * S;
    float c = 0.f;
    float gin = act ? a.gin[(row0 + (d ? S - 1 : 0)) * a.ldgin + (size_t)d * G + tid] : 0.f;
    for (int step = 0; step < S; ++step) {
        const int t = d ? S - 1 - step : step;
        const size_t row = row0 + t;
        float gin_next = 0.f;                                   // the next step's input term, loaded under this step
        if (act && step + 1 < S) gin_next = a.gin[(row0 + (d ? t - 1 : t + 1)) * a.ldgin + (size_t)d * G + tid];
        float acc0 = gin + bias, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
        for (int k = 0; k < HM; k += 4) {
            if (k < h) {
                const float4 hv = *reinterpret_cast<const float4*>(hs + k);
                acc0 = fmaf(w[k + 0], hv.x, acc0);
                acc1 = fmaf(w[k + 1], hv.y, acc1);
                acc2 = fmaf(w[k + 2], hv.z, acc2);
                acc3 = fmaf(w[k + 3], hv.w, acc3);
            }
        }
        const float pre = (acc0 + acc1) + (acc2 + acc3);
        const float gv = q == 2 ? tanhf(pre) : lstm_sigmoid(pre);
        if (act) {
            gs[tid] = gv;
            a.gates[row * a.ldgates + (size_t)d * G + tid] = gv;
        }
        __syncthreads();
        if (tid < h) {
            const float ig = gs[tid], fg = gs[h + tid], gg = gs[2 * h + tid], og = gs[3 * h + tid];
            const float hp = hs[tid];
            c = fg * c + ig * gg;
            const float hn = og * tanhf(c);
            a.hprev[row * a.ldhprev + (size_t)d * h + tid] = hp;
            a.cell[row * a.ldcell + (size_t)d * h + tid] = c;
            a.y[row * a.ldy + (size_t)d * h + tid] = hn;
            hs[tid] = hn;                                       // (every dot product of this step read hs before the barrier)
        }
        __syncthreads();
        gin = gin_next;
    }
}

template <int HM>
__global__ __launch_bounds__(512) void lstm_bwd_kernel(const LstmBwdArgs a) {
    __shared__ float dgs[4 * HM];                               // dG of the current step
    __shared__ float part[4 * HM];                              // [q][m]: dG_q . W_hh[q-block, m], summed by the next step
    const int h = a.h, G = 4 * h, S = a.S;
    const int b = (int)blockIdx.x >> 1, d = (int)blockIdx.x & 1;
    const int tid = (int)threadIdx.x;
    const bool act = tid < G;
    const int q = act ? tid / h : 0, m = act ? tid - q * h : 0;
    const float* W = d ? a.whh1 : a.whh0;
    float w[HM];                                                // w[jj] = W_hh[q h + jj, m]
#pragma unroll
    for (int k = 0; k < HM; k += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[k + e] = 0.f;
        if (act && k < h) {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[k + e] = W[(size_t)(q * h + k + e) * h + m];
        }
    }
    if (act) part[tid] = 0.f;
    __syncthreads();
    const size_t row0 = (size_t)b * S;
    const size_t gcol = (size_t)d * G, hcol = (size_t)d * h;
    float dc = 0.f;
    // the values of unit tid at backward step s (processing step S - 1 - s), prefetched one step ahead
    float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cc = 0.f, cp = 0.f, dyv = 0.f;
    auto load = [&](int s, float& i_, float& f_, float& g_, float& o_, float& c_, float& p_, float& y_) {
        const int tau = S - 1 - s;                              // processing step
        const int t = d ? S - 1 - tau : tau;
        const size_t row = row0 + t;
        const float* gr = a.gates + row * a.ldgates + gcol + tid;
        i_ = gr[0]; f_ = gr[h]; g_ = gr[2 * h]; o_ = gr[3 * h];
        c_ = a.cell[row * a.ldcell + hcol + tid];
        p_ = tau > 0 ? a.cell[(row0 + (d ? t + 1 : t - 1)) * a.ldcell + hcol + tid] : 0.f;
        y_ = a.dy[row * a.lddy + hcol + tid];
    };
    if (tid < h) load(0, ig, fg, gg, og, cc, cp, dyv);
    for (int s = 0; s < S; ++s) {
        const int tau = S - 1 - s;
        const int t = d ? S - 1 - tau : tau;
        const size_t row = row0 + t;
        if (tid < h) {
            float ni = 0.f, nf = 0.f, ng = 0.f, no = 0.f, nc = 0.f, np = 0.f, ny = 0.f;
            if (s + 1 < S) load(s + 1, ni, nf, ng, no, nc, np, ny);
            const float dh = dyv + ((part[tid] + part[h + tid]) + (part[2 * h + tid] + part[3 * h + tid]));
            const float tc = tanhf(cc);
            const float dct = dc + dh * og * (1.f - tc * tc);
            const float dgi = dct * gg * ig * (1.f - ig);
            const float dgf = dct * cp * fg * (1.f - fg);
            const float dgg = dct * ig * (1.f - gg * gg);
            const float dgo = dh * tc * og * (1.f - og);
            dc = dct * fg;
            dgs[tid] = dgi; dgs[h + tid] = dgf; dgs[2 * h + tid] = dgg; dgs[3 * h + tid] = dgo;
            float* o = a.dg + row * a.lddg + gcol + tid;
            o[0] = dgi; o[h] = dgf; o[2 * h] = dgg; o[3 * h] = dgo;
            ig = ni; fg = nf; gg = ng; og = no; cc = nc; cp = np; dyv = ny;
        }
        __syncthreads();
        if (act) {
            const float* src = dgs + q * h;
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
            for (int k = 0; k < HM; k += 4) {
                if (k < h) {
                    acc0 = fmaf(w[k + 0], src[k + 0], acc0);
                    acc1 = fmaf(w[k + 1], src[k + 1], acc1);
                    acc2 = fmaf(w[k + 2], src[k + 2], acc2);
                    acc3 = fmaf(w[k + 3], src[k + 3], acc3);
                }
            }
            part[tid] = (acc0 + acc1) + (acc2 + acc3);
        }
        __syncthreads();
    }
}

static int lstm_block(int h) { return ((4 * h + 63) / 64) * 64; }

}  // namespace r3d

using namespace r3d;

R3D_EXPORT int r3d_lstm_supported(int H) { return (H >= 8 && H <= 256 && H % 8 == 0) ? 1 : 0; }

R3D_EXPORT int r3d_lstm_layer_fwd(const float* gin, int ldgin, const float* whh_fwd, const float* whh_rev, const float* bhh_fwd,
                                  const float* bhh_rev, float* y, int ldy, float* gates, int ldgates, float* cell, int ldcell,
                                  float* hprev, int ldhprev, int B, int S, int H, void* stream) {
    R3D_REQUIRE(gin && whh_fwd && whh_rev && bhh_fwd && bhh_rev && y && gates && cell && hprev);
    R3D_REQUIRE(B > 0 && S > 0 && r3d_lstm_supported(H));
    const int h = H / 2;
    R3D_REQUIRE(ldgin >= 8 * h && ldgates >= 8 * h && ldy >= 2 * h && ldcell >= 2 * h && ldhprev >= 2 * h);
    const LstmFwdArgs a{gin, ldgin, whh_fwd, whh_rev, bhh_fwd, bhh_rev, y, ldy, gates, ldgates, cell, ldcell, hprev, ldhprev,
                        B, S, h};
    const dim3 grid(2 * B), block(lstm_block(h));
    if (h <= 32)
        hipLaunchKernelGGL(lstm_fwd_kernel<32>, grid, block, 0, (hipStream_t)stream, a);
    else if (h <= 64)
        hipLaunchKernelGGL(lstm_fwd_kernel<64>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(lstm_fwd_kernel<128>, grid, block, 0, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}

R3D_EXPORT int r3d_lstm_layer_bwd(const float* dy, int lddy, const float* whh_fwd, const float* whh_rev, const float* gates,
                                  int ldgates, const float* cell, int ldcell, float* dg, int lddg, int B, int S, int H,
                                  void* stream) {
    R3D_REQUIRE(dy && whh_fwd && whh_rev && gates && cell && dg);
    R3D_REQUIRE(B > 0 && S > 0 && r3d_lstm_supported(H));
    const int h = H / 2;
    R3D_REQUIRE(lddy >= 2 * h && ldgates >= 8 * h && ldcell >= 2 * h && lddg >= 8 * h);
    const LstmBwdArgs a{dy, lddy, whh_fwd, whh_rev, gates, ldgates, cell, ldcell, dg, lddg, B, S, h};
    const dim3 grid(2 * B), block(lstm_block(h));
    if (h <= 32)
        hipLaunchKernelGGL(lstm_bwd_kernel<32>, grid, block, 0, (hipStream_t)stream, a);
    else if (h <= 64)
        hipLaunchKernelGGL(lstm_bwd_kernel<64>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(lstm_bwd_kernel<128>, grid, block, 0, (hipStream_t)stream, a);
    R3D_LAUNCH_CHECK();
    return R3D_OK;
}
