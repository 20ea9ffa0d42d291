// Windows of F.adaptive_avg_pool1d over S rows down to Q: output q averages rows [pool_start(q), pool_end(q)) =
// [floor(q S / Q), ceil((q + 1) S / Q)).  Shared by the row kernels of posenc.hip and the pooled-head chain of afft.hip.
#pragma once

namespace r3d {

__device__ __forceinline__ int pool_start(int q, int S, int Q) { return (int)(((long long)q * S) / Q); }
__device__ __forceinline__ int pool_end(int q, int S, int Q) { return (int)((((long long)(q + 1)) * S + Q - 1) / Q); }

}  // namespace r3d
