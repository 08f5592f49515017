// MI355X (gfx950/CDNA4) native training kernels for mi355x_ddp.
//
// Implements the dependency-provided native pieces the reference relies on
// (SURVEY.md §2.2): fused BatchNorm(+Add)(+ReLU) forward/backward (N2),
// SyncBN local stats (N3), fused softmax-cross-entropy (N9), fused
// multi-tensor SGD with momentum+weight-decay (N9 north star), and the
// multi-tensor grad unscale + inf/nan check of the fp16 loss-scaler (N7).
//
// Written HIP-native for wave64/CDNA4 — no CUDA compat paths. Reductions use
// 64-lane shuffles + one LDS round per block; elementwise kernels are
// grid-stride. Compiled in-tree for gfx950 by csrc/build.py.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#define DEV static __device__ __forceinline__

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

namespace {

constexpr int WAVE = 64;  // CDNA wavefront width (gfx950)

DEV float warp_reduce_sum(float v) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WAVE);
  return v;
}

DEV float warp_reduce_max(float v) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, WAVE));
  return v;
}

// Block-level sum over up to 1024 threads (multiple waves) via LDS.
template <int MAX_WAVES = 16>
DEV float block_reduce_sum(float v, float* lds) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  v = warp_reduce_sum(v);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  const int nw = (blockDim.x + WAVE - 1) / WAVE;
  v = (threadIdx.x < nw) ? lds[threadIdx.x] : 0.f;
  if (wid == 0) v = warp_reduce_sum(v);
  return v;  // valid in thread 0
}

// ---------------------------------------------------------------------------
// BatchNorm statistics: per-channel sum and sum-of-squares over N,H,W (NCHW).
// Grid: (C, SPLIT) — SPLIT blocks stride over the N*S elements of channel c
// and atomically combine, so small-C stages still fill the chip's 256 CUs.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void bn_stats_kernel(const scalar_t* __restrict__ x,
                                float* __restrict__ sum,
                                float* __restrict__ sqsum,
                                int N, int C, int S) {
  __shared__ float lds[32];
  const int c = blockIdx.x;
  const long total = (long)N * S;
  float s = 0.f, sq = 0.f;
  for (long i = (long)blockIdx.y * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.y * blockDim.x) {
    const long n = i / S, sp = i % S;
    const float v = (float)x[(n * C + c) * S + sp];
    s += v;
    sq += v * v;
  }
  // two back-to-back block reductions share the LDS scratch
  s = block_reduce_sum(s, lds);
  __syncthreads();
  sq = block_reduce_sum(sq, lds);
  if (threadIdx.x == 0) {
    atomicAdd(&sum[c], s);
    atomicAdd(&sqsum[c], sq);
  }
}

// ---------------------------------------------------------------------------
// Fused BN forward: y = relu((x - mean) * invstd * w + b [+ residual])
// One elementwise pass; ATen would launch BN, add and ReLU separately.
// ---------------------------------------------------------------------------
template <typename scalar_t, bool RELU, bool HAS_RES, bool CLAST>
__global__ void bn_fwd_kernel(const scalar_t* __restrict__ x,
                              const scalar_t* __restrict__ res,
                              scalar_t* __restrict__ y,
                              const float* __restrict__ weight,
                              const float* __restrict__ bias,
                              const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              long total, int C, int S) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = CLAST ? (int)(i % C) : (int)((i / S) % C);
    float v = ((float)x[i] - mean[c]) * invstd[c] * weight[c] + bias[c];
    if (HAS_RES) v += (float)res[i];
    if (RELU) v = fmaxf(v, 0.f);
    y[i] = (scalar_t)v;
  }
}

// Vectorized variant: 8 elements (16 B) per thread. Correct when the
// channel run stays within one c-block: CLAST needs C %% 8 == 0, NCHW needs
// S %% 8 == 0 (true for every ResNet CIFAR stage).
// y = x*scale[c] + shift[c] (+res, relu): the four per-channel tables
// (mean/invstd/weight/bias) are pre-folded into two by bn_coeffs, and in
// CLAST mode the 8 consecutive channels load as two float4s.
// 4-deep unrolled grid-stride: the elementwise BN kernels are HBM-latency
// bound with one load in flight per lane; issuing 4 independent iterations'
// loads before any compute (Guideline 7: ILP for latency hiding) measured
// ~2x on the 224px tensors. Each sub-iteration stays wave-coalesced (the
// four v's are one grid-stride apart, not adjacent).
template <typename scalar_t, bool RELU, bool HAS_RES, bool CLAST>
__global__ void bn_fwd_vec_kernel(const scalar_t* __restrict__ x,
                                  const scalar_t* __restrict__ res,
                                  scalar_t* __restrict__ y,
                                  const float* __restrict__ scale,
                                  const float* __restrict__ shift,
                                  long nvec, int C, int S) {
  const long gstride = (long)gridDim.x * blockDim.x;
  for (long v0 = (long)blockIdx.x * blockDim.x + threadIdx.x; v0 < nvec;
       v0 += 4 * gstride) {
    scalar_t x8[4][8], r8[4][8], y8[4][8];
    float sc[4][8], sh[4][8];
    long iv[4];
    bool ok[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long v = v0 + k * gstride;
      ok[k] = v < nvec;
      iv[k] = v * 8;
      if (ok[k]) {
        *(float4*)x8[k] = *(const float4*)(x + iv[k]);
        if (HAS_RES) *(float4*)r8[k] = *(const float4*)(res + iv[k]);
      }
    }
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      if (CLAST) {
        const int c0 = (int)(iv[k] % C);
        *(float4*)&sc[k][0] = *(const float4*)(scale + c0);
        *(float4*)&sc[k][4] = *(const float4*)(scale + c0 + 4);
        *(float4*)&sh[k][0] = *(const float4*)(shift + c0);
        *(float4*)&sh[k][4] = *(const float4*)(shift + c0 + 4);
      } else {
        const int c = (int)((iv[k] / S) % C);
        #pragma unroll
        for (int e = 0; e < 8; ++e) { sc[k][e] = scale[c]; sh[k][e] = shift[c]; }
      }
    }
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        float o = (float)x8[k][e] * sc[k][e] + sh[k][e];
        if (HAS_RES) o += (float)r8[k][e];
        if (RELU) o = fmaxf(o, 0.f);
        y8[k][e] = (scalar_t)o;
      }
      *(float4*)(y + iv[k]) = *(float4*)y8[k];
    }
  }
}

// scale = w*invstd, shift = b - mean*scale (one tiny launch per BN forward)
__global__ void bn_coeffs_kernel(const float* __restrict__ weight,
                                 const float* __restrict__ bias,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ invstd,
                                 float* __restrict__ scale,
                                 float* __restrict__ shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = weight[c] * invstd[c];
  scale[c] = sc;
  shift[c] = bias[c] - mean[c] * sc;
}

// backward coefficient fold: dx = A[c]*g + B[c]*x + D[c]
//   A = w*is; B = -w*is^2*sum_dy_xhat/cnt; D = -A*sum_dy/cnt - B*mean
// (eval mode: B = D = 0 -> dx = A*g)
__global__ void bn_bwd_coeffs_kernel(const float* __restrict__ weight,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ invstd,
                                     const float* __restrict__ sum_dy,
                                     const float* __restrict__ sum_dy_xhat,
                                     float inv_count, bool training,
                                     float* __restrict__ A,
                                     float* __restrict__ B,
                                     float* __restrict__ D, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float is = invstd[c];
  const float a = weight[c] * is;
  float b = 0.f, dd = 0.f;
  if (training) {
    b = -a * is * sum_dy_xhat[c] * inv_count;
    dd = -a * sum_dy[c] * inv_count - b * mean[c];
  }
  A[c] = a;
  B[c] = b;
  D[c] = dd;
}

// ---------------------------------------------------------------------------
// BN backward reductions: per-channel sum_dy and sum_dy_xhat with the ReLU
// mask (y > 0) folded in — the fused-ReLU backward never materialises a mask.
// ---------------------------------------------------------------------------
template <typename scalar_t, bool RELU>
__global__ void bn_bwd_reduce_kernel(const scalar_t* __restrict__ dy,
                                     const scalar_t* __restrict__ x,
                                     const scalar_t* __restrict__ y,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ invstd,
                                     float* __restrict__ sum_dy,
                                     float* __restrict__ sum_dy_xhat,
                                     int N, int C, int S) {
  __shared__ float lds[32];
  const int c = blockIdx.x;
  const float mu = mean[c], is = invstd[c];
  const long total = (long)N * S;
  float sdy = 0.f, sdyx = 0.f;
  for (long i = (long)blockIdx.y * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.y * blockDim.x) {
    const long n = i / S, sp = i % S;
    const long idx = (n * C + c) * S + sp;
    float g = (float)dy[idx];
    if (RELU && (float)y[idx] <= 0.f) g = 0.f;
    sdy += g;
    sdyx += g * ((float)x[idx] - mu) * is;
  }
  sdy = block_reduce_sum(sdy, lds);
  __syncthreads();
  sdyx = block_reduce_sum(sdyx, lds);
  if (threadIdx.x == 0) {
    atomicAdd(&sum_dy[c], sdy);
    atomicAdd(&sum_dy_xhat[c], sdyx);
  }
}

// ---------------------------------------------------------------------------
// BN backward apply: dx (+ optional dresidual = relu-masked dy).
// training: dx = w*is*(g - sum_dy/cnt - xhat*sum_dy_xhat/cnt); eval: dx = w*is*g
// ---------------------------------------------------------------------------
template <typename scalar_t, bool RELU, bool TRAIN, bool NEED_DRES, bool CLAST>
__global__ void bn_bwd_kernel(const scalar_t* __restrict__ dy,
                              const scalar_t* __restrict__ x,
                              const scalar_t* __restrict__ y,
                              scalar_t* __restrict__ dx,
                              scalar_t* __restrict__ dres,
                              const float* __restrict__ weight,
                              const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const float* __restrict__ sum_dy,
                              const float* __restrict__ sum_dy_xhat,
                              float inv_count, long total, int C, int S) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = CLAST ? (int)(i % C) : (int)((i / S) % C);
    float g = (float)dy[i];
    if (RELU && (float)y[i] <= 0.f) g = 0.f;
    if (NEED_DRES) dres[i] = (scalar_t)g;
    const float w_is = weight[c] * invstd[c];
    float v;
    if (TRAIN) {
      const float xhat = ((float)x[i] - mean[c]) * invstd[c];
      v = w_is * (g - sum_dy[c] * inv_count - xhat * sum_dy_xhat[c] * inv_count);
    } else {
      v = w_is * g;
    }
    dx[i] = (scalar_t)v;
  }
}


// dx = A[c]*g + B[c]*x + D[c] with the relu mask on g; coefficient tables
// from bn_bwd_coeffs_kernel (eval: B=D=0).
// 2-deep unrolled (bwd reads up to 3 tensors per element — register
// pressure caps the depth; same latency-hiding rationale as bn_fwd_vec).
template <typename scalar_t, bool RELU, bool TRAIN, bool NEED_DRES, bool CLAST>
__global__ void bn_bwd_vec_kernel(const scalar_t* __restrict__ dy,
                                  const scalar_t* __restrict__ x,
                                  const scalar_t* __restrict__ y,
                                  scalar_t* __restrict__ dx,
                                  scalar_t* __restrict__ dres,
                                  const float* __restrict__ A,
                                  const float* __restrict__ B,
                                  const float* __restrict__ D,
                                  long nvec, int C, int S) {
  const long gstride = (long)gridDim.x * blockDim.x;
  for (long v0 = (long)blockIdx.x * blockDim.x + threadIdx.x; v0 < nvec;
       v0 += 2 * gstride) {
    scalar_t dy8[2][8], x8[2][8], y8[2][8], o8[8], dr8[8];
    long iv[2];
    bool ok[2];
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long v = v0 + k * gstride;
      ok[k] = v < nvec;
      iv[k] = v * 8;
      if (ok[k]) {
        *(float4*)dy8[k] = *(const float4*)(dy + iv[k]);
        if (TRAIN) *(float4*)x8[k] = *(const float4*)(x + iv[k]);
        if (RELU) *(float4*)y8[k] = *(const float4*)(y + iv[k]);
      }
    }
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!ok[k]) continue;
      const long i = iv[k];
      float a[8], b[8], dd[8];
      if (CLAST) {
        const int c0 = (int)(i % C);
        *(float4*)&a[0] = *(const float4*)(A + c0);
        *(float4*)&a[4] = *(const float4*)(A + c0 + 4);
        if (TRAIN) {
          *(float4*)&b[0] = *(const float4*)(B + c0);
          *(float4*)&b[4] = *(const float4*)(B + c0 + 4);
          *(float4*)&dd[0] = *(const float4*)(D + c0);
          *(float4*)&dd[4] = *(const float4*)(D + c0 + 4);
        }
      } else {
        const int c = (int)((i / S) % C);
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          a[e] = A[c];
          if (TRAIN) { b[e] = B[c]; dd[e] = D[c]; }
        }
      }
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        float g = (float)dy8[k][e];
        if (RELU && (float)y8[k][e] <= 0.f) g = 0.f;
        if (NEED_DRES) dr8[e] = (scalar_t)g;
        float o = a[e] * g;
        if (TRAIN) o += b[e] * (float)x8[k][e] + dd[e];
        o8[e] = (scalar_t)o;
      }
      *(float4*)(dx + i) = *(float4*)o8;
      if (NEED_DRES) *(float4*)(dres + i) = *(float4*)dr8;
    }
  }
}

// ---------------------------------------------------------------------------
// NHWC (channels_last) variants — the MI355X-preferred layout: per-pixel
// channels are contiguous, so stats/reductions coalesce across lanes on the
// channel axis and elementwise kernels compute c = i % C (pow2 on ResNet).
// MIOpen's tuned implicit-GEMM bf16 kernels are NHWC too, so the whole model
// runs channels_last with zero transposes.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void bn_stats_nhwc_kernel(const scalar_t* __restrict__ x,
                                     float* __restrict__ sum,
                                     float* __restrict__ sqsum,
                                     long P, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f, sq = 0.f;
  for (long p = blockIdx.y; p < P; p += gridDim.y) {
    const float v = (float)x[p * C + c];
    s += v;
    sq += v * v;
  }
  atomicAdd(&sum[c], s);
  atomicAdd(&sqsum[c], sq);
}

// v2: NHWC stats with full thread utilisation AND 16-byte loads. Each thread
// owns VEC=8 consecutive channels (one dwordx4 per pixel-row visited), tpr =
// C/8 threads span the channels, rpb = 256/tpr rows advance per iteration.
// The row axis folds with an LDS tree; each block writes its slice of
// partial[split][2C] — no atomics, no zero-init. Requires C % 8 == 0 (every
// ResNet BN); other C take the v1 atomic kernel.
typedef __attribute__((ext_vector_type(8))) __bf16 bnbf16x8;

template <typename scalar_t>
__global__ void bn_stats_nhwc_v2_kernel(const scalar_t* __restrict__ x,
                                        float* __restrict__ partial,  // [split][2C]
                                        long P, int C, int tpr) {
  __shared__ float lds[2 * 256 * 8];
  const int rpb = blockDim.x / tpr;
  const int c_idx = threadIdx.x % tpr;
  const int r = threadIdx.x / tpr;
  const int c0 = c_idx * 8;
  float s[8] = {}, sq[8] = {};
  // 4 rows per loop pass: the loads are issued together (independent) so
  // up to 4 HBM fetches overlap instead of one latency per row
  const long pstride = (long)gridDim.y * rpb;
  for (long p0 = (long)blockIdx.y * rpb + r; p0 < P; p0 += 4 * pstride) {
    scalar_t v8[4][8];
    bool ok[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long p = p0 + k * pstride;
      ok[k] = p < P;
      if (!ok[k]) continue;
      if constexpr (sizeof(scalar_t) == 2) {
        *(float4*)v8[k] = *(const float4*)(x + p * C + c0);
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e) v8[k][e] = x[p * C + c0 + e];
      }
    }
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = (float)v8[k][e];
        s[e] += v;
        sq[e] += v * v;
      }
    }
  }
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    lds[threadIdx.x * 8 + e] = s[e];
    lds[2048 + threadIdx.x * 8 + e] = sq[e];
  }
  // fold rows: tree over the r axis (threads r, r+stride share c_idx)
  for (int stride = rpb >> 1; stride > 0; stride >>= 1) {
    __syncthreads();
    if (r < stride) {
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        lds[threadIdx.x * 8 + e] += lds[(threadIdx.x + stride * tpr) * 8 + e];
        lds[2048 + threadIdx.x * 8 + e] +=
            lds[2048 + (threadIdx.x + stride * tpr) * 8 + e];
      }
    }
  }
  __syncthreads();
  if (r == 0) {
    float* row = partial + (long)blockIdx.y * 2 * C;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      row[c0 + e] = lds[threadIdx.x * 8 + e];
      row[C + c0 + e] = lds[2048 + threadIdx.x * 8 + e];
    }
  }
}

// partial [split][2C] -> packed [2C]: one block per output element, the
// split axis reduced by 256 threads (split <= 512 -> <=2 loads per thread).
__global__ void bn_reduce_partials_kernel(const float* __restrict__ partial,
                                          float* __restrict__ packed,
                                          int split, int twoC) {
  __shared__ float lds[32];
  const int i = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < split; j += blockDim.x)
    s += partial[(long)j * twoC + i];
  s = block_reduce_sum(s, lds);
  if (threadIdx.x == 0) packed[i] = s;
}

// packed {sum, sqsum} + count -> mean, invstd (+ running stats update).
// Replaces the ~10 ATen launches of eager mean/var/rsqrt/lerp per BN layer.
__global__ void bn_finalize_kernel(const float* __restrict__ packed,
                                   float* __restrict__ mean_out,
                                   float* __restrict__ invstd_out,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   float count, float momentum, float eps,
                                   int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float mean = packed[c] / count;
  float var = packed[C + c] / count - mean * mean;
  var = fmaxf(var, 0.f);
  mean_out[c] = mean;
  invstd_out[c] = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    const float unbiased = var * (count / fmaxf(count - 1.f, 1.f));
    running_mean[c] += momentum * (mean - running_mean[c]);
    running_var[c] += momentum * (unbiased - running_var[c]);
  }
}

// Forward tail: partial [split][2C] -> stats [4][C] = {mean, invstd, scale,
// shift} (+ running stats update) in ONE launch, replacing the
// bn_reduce_partials -> bn_finalize -> bn_coeffs chain. Block c folds the sum
// and sqsum columns of channel c in bn_reduce_partials_kernel's order (thread-
// strided j loop at 256 threads, then block_reduce_sum) and thread 0 applies
// the bn_finalize_kernel / bn_coeffs_kernel expressions unchanged, so the
// results are bit-identical to the three-kernel chain. split == 1 (a packed
// [2C] after the SyncBN all_reduce) is the degenerate case of the same loop.
__global__ void bn_fwd_tail_kernel(const float* __restrict__ partial,
                                   const float* __restrict__ weight,
                                   const float* __restrict__ bias,
                                   float* __restrict__ stats,  // [4][C]
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   float count, float momentum, float eps,
                                   int split, int C) {
  __shared__ float lds[32];
  const int c = blockIdx.x;
  const int twoC = 2 * C;
  float s = 0.f, sq = 0.f;
  for (int j = threadIdx.x; j < split; j += blockDim.x) {
    s += partial[(long)j * twoC + c];
    sq += partial[(long)j * twoC + C + c];
  }
  s = block_reduce_sum(s, lds);
  __syncthreads();
  sq = block_reduce_sum(sq, lds);
  if (threadIdx.x != 0) return;
  const float mean = s / count;
  float var = sq / count - mean * mean;
  var = fmaxf(var, 0.f);
  const float invstd = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    const float unbiased = var * (count / fmaxf(count - 1.f, 1.f));
    running_mean[c] += momentum * (mean - running_mean[c]);
    running_var[c] += momentum * (unbiased - running_var[c]);
  }
  const float sc = weight[c] * invstd;
  stats[c] = mean;
  stats[C + c] = invstd;
  stats[2 * C + c] = sc;
  stats[3 * C + c] = bias[c] - mean * sc;
}

// Backward tail: partial [split][2C] -> sums [2][C] = {sum_dy, sum_dy_xhat}
// (dbeta, dgamma of the local batch) and, in the same launch, either the
// bn_bwd_coeffs_kernel fold into coeffs [3][C] = {A, B, D}, or (DUP) a second
// copy of the sums as packed [2C] for the SyncBN all_reduce to overwrite.
// Reduction order as in bn_fwd_tail_kernel.
template <bool DUP>
__global__ void bn_bwd_tail_kernel(const float* __restrict__ partial,
                                   const float* __restrict__ weight,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ invstd,
                                   float inv_count, bool training,
                                   float* __restrict__ sums,  // [2][C]
                                   float* __restrict__ out,   // [3][C] | [2C]
                                   int split, int C) {
  __shared__ float lds[32];
  const int c = blockIdx.x;
  const int twoC = 2 * C;
  float sdy = 0.f, sdyx = 0.f;
  for (int j = threadIdx.x; j < split; j += blockDim.x) {
    sdy += partial[(long)j * twoC + c];
    sdyx += partial[(long)j * twoC + C + c];
  }
  sdy = block_reduce_sum(sdy, lds);
  __syncthreads();
  sdyx = block_reduce_sum(sdyx, lds);
  if (threadIdx.x != 0) return;
  sums[c] = sdy;
  sums[C + c] = sdyx;
  if (DUP) {
    out[c] = sdy;
    out[C + c] = sdyx;
    return;
  }
  const float is = invstd[c];
  const float a = weight[c] * is;
  float b = 0.f, dd = 0.f;
  if (training) {
    b = -a * is * sdyx * inv_count;
    dd = -a * sdy * inv_count - b * mean[c];
  }
  out[c] = a;
  out[C + c] = b;
  out[2 * C + c] = dd;
}

template <typename scalar_t, bool RELU>
__global__ void bn_bwd_reduce_nhwc_v2_kernel(const scalar_t* __restrict__ dy,
                                             const scalar_t* __restrict__ x,
                                             const scalar_t* __restrict__ y,
                                             const float* __restrict__ mean,
                                             const float* __restrict__ invstd,
                                             float* __restrict__ partial,  // [split][2C]
                                             long P, int C, int tpr) {
  __shared__ float lds[2 * 256 * 8];
  const int rpb = blockDim.x / tpr;
  const int c_idx = threadIdx.x % tpr;
  const int r = threadIdx.x / tpr;
  const int c0 = c_idx * 8;
  float mu[8], is[8];
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu[e] = mean[c0 + e];
    is[e] = invstd[c0 + e];
  }
  float sdy[8] = {}, sdyx[8] = {};
  // 2 rows per pass (2-3 tensors each): 4-6 fetches in flight
  const long pstride = (long)gridDim.y * rpb;
  for (long p0 = (long)blockIdx.y * rpb + r; p0 < P; p0 += 2 * pstride) {
    scalar_t dy8[2][8], x8[2][8], y8[2][8];
    bool ok[2];
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long p = p0 + k * pstride;
      ok[k] = p < P;
      if (!ok[k]) continue;
      const long base = p * C + c0;
      if constexpr (sizeof(scalar_t) == 2) {
        *(float4*)dy8[k] = *(const float4*)(dy + base);
        *(float4*)x8[k] = *(const float4*)(x + base);
        if (RELU) *(float4*)y8[k] = *(const float4*)(y + base);
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          dy8[k][e] = dy[base + e];
          x8[k][e] = x[base + e];
          if (RELU) y8[k][e] = y[base + e];
        }
      }
    }
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!ok[k]) continue;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        float g = (float)dy8[k][e];
        if (RELU && (float)y8[k][e] <= 0.f) g = 0.f;
        sdy[e] += g;
        sdyx[e] += g * ((float)x8[k][e] - mu[e]) * is[e];
      }
    }
  }
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    lds[threadIdx.x * 8 + e] = sdy[e];
    lds[2048 + threadIdx.x * 8 + e] = sdyx[e];
  }
  for (int stride = rpb >> 1; stride > 0; stride >>= 1) {
    __syncthreads();
    if (r < stride) {
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        lds[threadIdx.x * 8 + e] += lds[(threadIdx.x + stride * tpr) * 8 + e];
        lds[2048 + threadIdx.x * 8 + e] +=
            lds[2048 + (threadIdx.x + stride * tpr) * 8 + e];
      }
    }
  }
  __syncthreads();
  if (r == 0) {
    float* row = partial + (long)blockIdx.y * 2 * C;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      row[c0 + e] = lds[threadIdx.x * 8 + e];
      row[C + c0 + e] = lds[2048 + threadIdx.x * 8 + e];
    }
  }
}

template <typename scalar_t, bool RELU>
__global__ void bn_bwd_reduce_nhwc_kernel(const scalar_t* __restrict__ dy,
                                          const scalar_t* __restrict__ x,
                                          const scalar_t* __restrict__ y,
                                          const float* __restrict__ mean,
                                          const float* __restrict__ invstd,
                                          float* __restrict__ sum_dy,
                                          float* __restrict__ sum_dy_xhat,
                                          long P, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float mu = mean[c], is = invstd[c];
  float sdy = 0.f, sdyx = 0.f;
  for (long p = blockIdx.y; p < P; p += gridDim.y) {
    const long idx = p * C + c;
    float g = (float)dy[idx];
    if (RELU && (float)y[idx] <= 0.f) g = 0.f;
    sdy += g;
    sdyx += g * ((float)x[idx] - mu) * is;
  }
  atomicAdd(&sum_dy[c], sdy);
  atomicAdd(&sum_dy_xhat[c], sdyx);
}

// ---------------------------------------------------------------------------
// Fused softmax + cross entropy (mean reduction). One block per row computes
// max, sum(exp), lse and the NLL contribution in a single pass over C classes.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void xent_fwd_kernel(const scalar_t* __restrict__ logits,
                                const long* __restrict__ target,
                                float* __restrict__ lse_out,
                                float* __restrict__ row_loss,
                                int N, int C) {
  __shared__ float lds[32];
  const int row = blockIdx.x;
  const scalar_t* xr = logits + (long)row * C;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < C; j += blockDim.x)
    m = fmaxf(m, (float)xr[j]);
  // block max: reuse sum-reduction structure with max
  {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    m = warp_reduce_max(m);
    if (lane == 0) lds[wid] = m;
    __syncthreads();
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    float v = (threadIdx.x < nw) ? lds[threadIdx.x] : -INFINITY;
    if (wid == 0) v = warp_reduce_max(v);
    if (threadIdx.x == 0) lds[31] = v;
    __syncthreads();
    m = lds[31];
  }
  __syncthreads();
  float s = 0.f;
  for (int j = threadIdx.x; j < C; j += blockDim.x)
    s += __expf((float)xr[j] - m);
  s = block_reduce_sum(s, lds);
  if (threadIdx.x == 0) {
    const float lse = m + __logf(s);
    lse_out[row] = lse;
    row_loss[row] = (lse - (float)xr[target[row]]) / N;
  }
}

// Sum of the per-row contributions in a fixed order (one block, strided
// partials then the shuffle tree), so the scalar loss is the same bits for
// the same logits (the atomicAdd per row this replaces summed in arrival
// order and moved the last bits from run to run). It takes the place of the
// memset that accumulator needed, so the launch count is unchanged.
__global__ void xent_mean_kernel(const float* __restrict__ row_loss,
                                 float* __restrict__ loss_out, int N) {
  __shared__ float lds[32];
  float s = 0.f;
  for (int j = threadIdx.x; j < N; j += blockDim.x) s += row_loss[j];
  s = block_reduce_sum(s, lds);
  if (threadIdx.x == 0) *loss_out = s;
}

template <typename scalar_t>
__global__ void xent_bwd_kernel(const scalar_t* __restrict__ logits,
                                const long* __restrict__ target,
                                const float* __restrict__ lse,
                                const float* __restrict__ dloss,
                                scalar_t* __restrict__ dx,
                                long total, int C) {
  const float scale = dloss[0];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / C;
    const int col = (int)(i % C);
    float p = __expf((float)logits[i] - lse[row]);
    if (col == (int)target[row]) p -= 1.f;
    dx[i] = (scalar_t)(p * scale / (total / C));
  }
}

// ---------------------------------------------------------------------------
// Two-label smoothed cross entropy (CutMix targets + label smoothing):
//   q_r  = (1-eps) * (l*x[r,a] + (1-l)*x[r,b]) + (eps/C) * sum_j x[r,j]
//   loss = mean_r (lse_r - q_r)
// i.e. l*CE(x,a) + (1-l)*CE(x,b) with torch's label_smoothing=eps. The max /
// sum(exp) / lse part is xent_fwd_kernel's, statement for statement; the row
// sum of x is a third block reduction in the same pass. Keep q in the form
// above: with l = 1 and eps = 0 it is 1*xa + 0*xb + 0*sum == xa exactly, so
// the kernel then gives xent_fwd_kernel's bits for any finite logits and any b.
// A class outside [0, C) reads nothing and counts as a zero logit.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void xent_mix_fwd_kernel(const scalar_t* __restrict__ logits,
                                    const long* __restrict__ target_a,
                                    const long* __restrict__ target_b,
                                    const float* __restrict__ lam,
                                    float* __restrict__ lse_out,
                                    float* __restrict__ row_loss,
                                    float eps, int N, int C) {
  __shared__ float lds[32];
  const int row = blockIdx.x;
  const scalar_t* xr = logits + (long)row * C;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < C; j += blockDim.x)
    m = fmaxf(m, (float)xr[j]);
  {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    m = warp_reduce_max(m);
    if (lane == 0) lds[wid] = m;
    __syncthreads();
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    float v = (threadIdx.x < nw) ? lds[threadIdx.x] : -INFINITY;
    if (wid == 0) v = warp_reduce_max(v);
    if (threadIdx.x == 0) lds[31] = v;
    __syncthreads();
    m = lds[31];
  }
  __syncthreads();
  float s = 0.f, sx = 0.f;
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const float x = (float)xr[j];
    s += __expf(x - m);
    sx += x;
  }
  s = block_reduce_sum(s, lds);
  __syncthreads();  // lds is reused by the next reduction
  sx = block_reduce_sum(sx, lds);
  if (threadIdx.x == 0) {
    const float lse = m + __logf(s);
    lse_out[row] = lse;
    const long a = target_a[row], b = target_b[row];
    const float xa = (unsigned long)a < (unsigned long)C ? (float)xr[a] : 0.f;
    const float xb = (unsigned long)b < (unsigned long)C ? (float)xr[b] : 0.f;
    const float l = lam[row];
    const float q = (1.f - eps) * (l * xa + (1.f - l) * xb) + (eps / C) * sx;
    row_loss[row] = (lse - q) / N;
  }
}

// dx = (softmax(x) - (1-eps)*(l*[j==a] + (1-l)*[j==b]) - eps/C) * dloss / N;
// a == b adds both one-hots. With l = 1, eps = 0 the subtracted terms are
// exactly 1 or 0 and 0, which is xent_bwd_kernel's arithmetic.
template <typename scalar_t>
__global__ void xent_mix_bwd_kernel(const scalar_t* __restrict__ logits,
                                    const long* __restrict__ target_a,
                                    const long* __restrict__ target_b,
                                    const float* __restrict__ lam,
                                    const float* __restrict__ lse,
                                    const float* __restrict__ dloss,
                                    scalar_t* __restrict__ dx,
                                    float eps, long total, int C) {
  const float scale = dloss[0];
  const float eps_c = eps / C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / C;
    const int col = (int)(i % C);
    float p = __expf((float)logits[i] - lse[row]);
    const float l = lam[row];
    const float ia = col == (int)target_a[row] ? 1.f : 0.f;
    const float ib = col == (int)target_b[row] ? 1.f : 0.f;
    const float t = (1.f - eps) * (l * ia + (1.f - l) * ib);
    p = p - t - eps_c;
    dx[i] = (scalar_t)(p * scale / (total / C));
  }
}

// ---------------------------------------------------------------------------
// Multi-tensor kernels: one launch works on up to MT_MAX_TENSORS tensors, one
// 256-thread block per MT_CHUNK elements of each. Tensor pointers travel in
// kernel-arg space (no host->device table copies); each block linear-scans
// the per-tensor chunk counts to find its tensor (mt_locate).
// ---------------------------------------------------------------------------
constexpr int MT_MAX_TENSORS = 32;
constexpr int MT_CHUNK = 1 << 13;

template <typename int_t>
__host__ __device__ constexpr int_t mt_chunks(int_t numel) {
  return (numel + MT_CHUNK - 1) / MT_CHUNK;
}

// Tensor t and its elements [start, end) of this block, for any of the list
// structs below. False when the block is past the launch's last chunk.
template <typename List>
__device__ __forceinline__ bool mt_locate(const List& tl, int& t, int& start,
                                          int& end) {
  int b = blockIdx.x;
  for (t = 0; t < tl.ntensors; ++t) {
    const int nchunks = mt_chunks(tl.size[t]);
    if (b < nchunks) break;
    b -= nchunks;
  }
  if (t >= tl.ntensors) return false;
  start = b * MT_CHUNK;
  end = min(start + MT_CHUNK, tl.size[t]);
  return true;
}

// ---------------------------------------------------------------------------
// SGD with momentum + weight decay on one element, w the fp32 weight:
//   plain   d = g + wd*w                 (exact torch.optim.SGD math)
//   SCALED  d = rt * (c*g + wd*w)        (c, rt from sgd_coeffs_kernel)
//   m <- mu*m + d  (when has_momentum) ; returns w - lr*d
// There is exactly one of these, inlined into the vector and the scalar loop
// of the fp32 kernel and into the O2 kernel: every bit of w and m must agree
// between the vector and the scalar path, and between a step with shadows and
// one without. The FMAs are written out because contraction left to the
// compiler differs between call sites: it turns c*g + wd*w into
// fma(c, g, wd*w) in the vector loop but, in a scalar loop where it first
// packs c*g and wd*w into one v_pk_mul_f32, into an unfused add. m is not
// read or written when has_momentum is false.
// ---------------------------------------------------------------------------
template <bool SCALED>
__device__ __forceinline__ float sgd_update(float w, float g, float& m,
                                            bool has_momentum, float lr,
                                            float mu, float wd, float c,
                                            float rt) {
  float d = SCALED ? rt * fmaf(c, g, wd * w) : fmaf(wd, w, g);
  if (has_momentum) {
    d = fmaf(mu, m, d);
    m = d;
  }
  return fmaf(-lr, d, w);
}

// Exponential moving average of a weight on one element: e <- d*e + omd*w,
// with omd = 1.f - d formed once on the host. Exact at both ends: d = 0 gives
// w bit for bit (0*e + w), d = 1 leaves e. One definition for the vector and
// the scalar loop of the fp32 SGD kernel, the O2 kernel and multi_tensor_ema;
// the fmaf is written out for the reason given above sgd_update.
__device__ __forceinline__ float ema_update(float e, float w, float d,
                                            float omd) {
  return fmaf(d, e, omd * w);
}

// w16[t], where not null, is a 16-bit shadow of p[t] in the same memory order
// (the conv layers' autocast copy of an fp32 weight): the kernel that produces
// the new weight also stores its rounded copy, so no cast kernel runs per
// forward. w16_half[t] gives the shadow's format, fp16 or bf16, per tensor:
// one step may refresh both kinds. The rounding is the float -> 16-bit
// conversion's round-to-nearest-even, as in ATen's copy kernel. The flag only
// selects the shadow store; the update arithmetic does not see it.
// ema[t], where not null, is the tensor's averaged weight (ema_update); only
// the EMA instantiations read it. sizeof(MTTensorList) = 5*256 + 128 + 32 + 4
// = 1444 -> 1448 bytes of the 4 KiB of kernel-argument space.
struct MTTensorList {
  float* p[MT_MAX_TENSORS];
  float* g[MT_MAX_TENSORS];
  float* m[MT_MAX_TENSORS];
  void* w16[MT_MAX_TENSORS];
  float* ema[MT_MAX_TENSORS];
  int size[MT_MAX_TENSORS];
  bool w16_half[MT_MAX_TENSORS];
  int ntensors;
};

typedef __attribute__((ext_vector_type(4))) __bf16 mtbf16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 mthalfx4;

// fp32 params. SCALED reads the clip coefficient gscale[0] and the per-tensor
// ratio[t] from device memory; g is not modified. A tensor whose pointers are
// all 16-byte aligned (8 for w16) moves as float4s; any other, and the last
// size % 4 elements, go element by element. EMA also averages the new weight
// into ema[t] (decay d, omd = 1 - d) where that is not null; without EMA the
// kernel does not touch tl.ema, d or omd.
template <bool SCALED, bool EMA>
__global__ void multi_tensor_sgd_kernel(MTTensorList tl, float lr, float mu,
                                        float wd, bool has_momentum,
                                        const float* __restrict__ gscale,
                                        const float* __restrict__ ratio,
                                        float d, float omd) {
  int t, start, end;
  if (!mt_locate(tl, t, start, end)) return;
  const float c = SCALED ? gscale[0] : 1.f;
  const float rt = SCALED ? ratio[t] : 1.f;
  float* p = tl.p[t];
  float* g = tl.g[t];
  float* m = has_momentum ? tl.m[t] : nullptr;
  void* w16 = tl.w16[t];
  float* ema = EMA ? tl.ema[t] : nullptr;
  const bool half = tl.w16_half[t];
  const bool vec = (((size_t)p | (size_t)g | (size_t)m | (size_t)ema) & 15)
                       == 0 &&
                   ((size_t)w16 & 7) == 0;
  int tail = start;   // first element of the scalar loop
  if (vec) {
    // start is a multiple of MT_CHUNK, so every float4 below is aligned
    tail = start + ((end - start) & ~3);
    for (int i = start + 4 * threadIdx.x; i < tail; i += 4 * blockDim.x) {
      float pv[4], gv[4], mv[4], ev[4];
      *(float4*)pv = *(const float4*)(p + i);
      *(float4*)gv = *(const float4*)(g + i);
      if (has_momentum) *(float4*)mv = *(const float4*)(m + i);
      // with the other loads: after the stores to m and p, which might alias
      // it for all the compiler knows, this load could not move up here
      if (EMA && ema != nullptr) *(float4*)ev = *(const float4*)(ema + i);
      #pragma unroll
      for (int e = 0; e < 4; ++e)
        pv[e] = sgd_update<SCALED>(pv[e], gv[e], mv[e], has_momentum, lr, mu,
                                   wd, c, rt);
      if (has_momentum) *(float4*)(m + i) = *(float4*)mv;
      *(float4*)(p + i) = *(float4*)pv;
      if (EMA && ema != nullptr) {
        #pragma unroll
        for (int e = 0; e < 4; ++e) ev[e] = ema_update(ev[e], pv[e], d, omd);
        *(float4*)(ema + i) = *(float4*)ev;
      }
      if (w16 != nullptr) {
        if (half) {
          mthalfx4 o;
          #pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)pv[e];
          *(mthalfx4*)((_Float16*)w16 + i) = o;
        } else {
          mtbf16x4 o;
          #pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (__bf16)pv[e];
          *(mtbf16x4*)((__bf16*)w16 + i) = o;
        }
      }
    }
  }
  for (int i = tail + threadIdx.x; i < end; i += blockDim.x) {
    float mv = 0.f;
    if (has_momentum) mv = m[i];
    const float pn = sgd_update<SCALED>(p[i], g[i], mv, has_momentum, lr, mu,
                                        wd, c, rt);
    if (has_momentum) m[i] = mv;
    p[i] = pn;
    if (EMA && ema != nullptr) ema[i] = ema_update(ema[i], pn, d, omd);
    if (w16 != nullptr) {
      if (half) ((_Float16*)w16)[i] = (_Float16)pn;
      else ((__bf16*)w16)[i] = (__bf16)pn;
    }
  }
}

// ---------------------------------------------------------------------------
// Mixed-precision multi-tensor SGD (apex O2 equivalent): bf16 model
// weights + bf16 grads + fp32 MASTER weights and momentum. sgd_update runs
// in fp32 against the master; the bf16 parameter is the rounded copy.
// ---------------------------------------------------------------------------
struct MTMixedList {
  __bf16* p[MT_MAX_TENSORS];
  const __bf16* g[MT_MAX_TENSORS];
  float* w[MT_MAX_TENSORS];   // master
  float* m[MT_MAX_TENSORS];
  float* ema[MT_MAX_TENSORS];   // average of the master, or null (EMA only)
  int size[MT_MAX_TENSORS];
  int ntensors;
};   // 5*256 + 128 + 4 = 1412 -> 1416 bytes of kernel-argument space

template <bool SCALED, bool EMA>
__global__ void multi_tensor_sgd_o2_kernel(MTMixedList tl, float lr, float mu,
                                           float wd, bool has_momentum,
                                           const float* __restrict__ gscale,
                                           const float* __restrict__ ratio,
                                           float d, float omd) {
  int t, start, end;
  if (!mt_locate(tl, t, start, end)) return;
  const float c = SCALED ? gscale[0] : 1.f;
  const float rt = SCALED ? ratio[t] : 1.f;
  __bf16* p = tl.p[t];
  const __bf16* g = tl.g[t];
  float* w = tl.w[t];
  float* m = has_momentum ? tl.m[t] : nullptr;
  float* ema = EMA ? tl.ema[t] : nullptr;
  for (int i = start + threadIdx.x; i < end; i += blockDim.x) {
    float mv = 0.f;
    if (has_momentum) mv = m[i];
    const float nw = sgd_update<SCALED>(w[i], (float)g[i], mv, has_momentum,
                                        lr, mu, wd, c, rt);
    if (has_momentum) m[i] = mv;
    w[i] = nw;
    p[i] = (__bf16)nw;
    if (EMA && ema != nullptr) ema[i] = ema_update(ema[i], nw, d, omd);
  }
}

// ---------------------------------------------------------------------------
// ema[t] <- d*ema[t] + omd*src[t] for tensors the optimizer does not step
// (the BatchNorm running statistics). fp32 both; float4s when both pointers
// are 16-byte aligned, element by element otherwise and for the last
// size % 4. src is not modified.
// ---------------------------------------------------------------------------
struct MTEmaList {
  const float* src[MT_MAX_TENSORS];
  float* ema[MT_MAX_TENSORS];
  int size[MT_MAX_TENSORS];
  int ntensors;
};

__global__ void multi_tensor_ema_kernel(MTEmaList tl, float d, float omd) {
  int t, start, end;
  if (!mt_locate(tl, t, start, end)) return;
  const float* src = tl.src[t];
  float* ema = tl.ema[t];
  int tail = start;
  if ((((size_t)src | (size_t)ema) & 15) == 0) {
    // start is a multiple of MT_CHUNK, so every float4 below is aligned
    tail = start + ((end - start) & ~3);
    for (int i = start + 4 * threadIdx.x; i < tail; i += 4 * blockDim.x) {
      float sv[4], ev[4];
      *(float4*)sv = *(const float4*)(src + i);
      *(float4*)ev = *(const float4*)(ema + i);
      #pragma unroll
      for (int e = 0; e < 4; ++e) ev[e] = ema_update(ev[e], sv[e], d, omd);
      *(float4*)(ema + i) = *(float4*)ev;
    }
  }
  for (int i = tail + threadIdx.x; i < end; i += blockDim.x)
    ema[i] = ema_update(ema[i], src[i], d, omd);
}

// ---------------------------------------------------------------------------
// Per-tensor squared L2 norms of weights and gradients, for LARS and for
// clipping by the global gradient norm. Same chunking as the SGD kernel: block
// b reduces chunk b of its tensor and stores the two sums at its global chunk
// index in `partials` ([2][total_chunks]: weights, then gradients); the fold
// kernel, one block per tensor, sums a tensor's partials into sq ([2][n]).
// No atomics: every sum has a fixed order, so two runs agree bit for bit.
// w is fp32 (the parameter or the O2 master); g is fp32 or bf16.
//
// Additions on the longest path to one sq value: MT_CHUNK/256 = 32 in a
// thread, 6 + 6 in block_reduce_sum, then ceil(nchunks/256) in a fold thread
// and 6 + 6 again: 56 + ceil(nchunks/256).
// ---------------------------------------------------------------------------
struct MTNormList {
  const float* w[MT_MAX_TENSORS];
  const void* g[MT_MAX_TENSORS];
  int size[MT_MAX_TENSORS];
  int ntensors;
};

template <typename grad_t>
__global__ void multi_tensor_sqnorm_kernel(MTNormList tl,
                                           float* __restrict__ partials,
                                           int chunk_base, int total_chunks) {
  __shared__ float lds[32];
  // 16 bytes of gradient per load: 4 floats or 8 bf16
  constexpr int VEC = 16 / sizeof(grad_t);
  typedef __attribute__((ext_vector_type(VEC))) grad_t gvec_t;
  int t, start, end;
  if (!mt_locate(tl, t, start, end)) return;
  const float* w = tl.w[t];
  const grad_t* g = (const grad_t*)tl.g[t];
  float sw = 0.f, sg = 0.f;
  int tail = start;   // first element of the scalar loop
  if ((((size_t)w | (size_t)g) & 15) == 0) {
    // start is a multiple of MT_CHUNK, so every 16-byte load is aligned
    tail = start + ((end - start) & ~(VEC - 1));
    for (int i = start + VEC * threadIdx.x; i < tail; i += VEC * blockDim.x) {
      float wv[VEC];
      #pragma unroll
      for (int e = 0; e < VEC; e += 4)
        *(float4*)(wv + e) = *(const float4*)(w + i + e);
      const gvec_t gv = *(const gvec_t*)(g + i);
      #pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float gf = (float)gv[e];
        sw += wv[e] * wv[e];
        sg += gf * gf;
      }
    }
  }
  for (int i = tail + threadIdx.x; i < end; i += blockDim.x) {
    const float wf = w[i];
    const float gf = (float)g[i];
    sw += wf * wf;
    sg += gf * gf;
  }
  sw = block_reduce_sum(sw, lds);
  __syncthreads();
  sg = block_reduce_sum(sg, lds);
  if (threadIdx.x == 0) {
    partials[chunk_base + blockIdx.x] = sw;
    partials[total_chunks + chunk_base + blockIdx.x] = sg;
  }
}

// Block t sums the partials of tensor t of this launch: strided over the
// block's threads, then block_reduce_sum.
__global__ void multi_tensor_sqnorm_fold_kernel(MTNormList tl,
                                                const float* __restrict__ partials,
                                                float* __restrict__ sq,
                                                int chunk_base, int total_chunks,
                                                int tensor_base, int n) {
  __shared__ float lds[32];
  const int t = blockIdx.x;
  if (t >= tl.ntensors) return;
  int off = chunk_base;
  for (int u = 0; u < t; ++u) off += mt_chunks(tl.size[u]);
  const int nchunks = mt_chunks(tl.size[t]);
  float sw = 0.f, sg = 0.f;
  for (int j = threadIdx.x; j < nchunks; j += blockDim.x) {
    sw += partials[off + j];
    sg += partials[total_chunks + off + j];
  }
  sw = block_reduce_sum(sw, lds);
  __syncthreads();
  sg = block_reduce_sum(sg, lds);
  if (threadIdx.x == 0) {
    sq[tensor_base + t] = sw;
    sq[n + tensor_base + t] = sg;
  }
}

// ---------------------------------------------------------------------------
// sq -> the coefficients of the scaled SGD step, one block:
//   norm     = sqrt(sum_t sq_g[t])                 (t in index order)
//   c        = min(1, max_norm / (norm + CLIP_EPS))   1 when max_norm <= 0
//   ratio[t] = eta*|w_t| / (c*|g_t| + wd*|w_t| + LARS_EPS)
// ratio[t] is 1 when LARS is off, when t is flagged excluded, and when |w_t|
// or |g_t| is 0. c is torch.nn.utils.clip_grad_norm_'s coefficient. The sum
// covers all n tensors; ratios are written for [lo, hi) only, so that param
// groups with different settings share one global norm.
// ---------------------------------------------------------------------------
constexpr float CLIP_EPS = 1e-6f;
constexpr float LARS_EPS = 1e-8f;

__global__ void sgd_coeffs_kernel(const float* __restrict__ sq,
                                  const unsigned char* __restrict__ excluded,
                                  float* __restrict__ gscale,
                                  float* __restrict__ ratio,
                                  float* __restrict__ gnorm,
                                  int n, int lo, int hi, float max_norm,
                                  bool lars, float eta, float wd) {
  __shared__ float c_sh;
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int t = 0; t < n; ++t) total += sq[n + t];
    const float norm = sqrtf(total);
    const float c = max_norm > 0.f
        ? fminf(1.f, max_norm / (norm + CLIP_EPS)) : 1.f;
    gscale[0] = c;
    gnorm[0] = norm;
    c_sh = c;
  }
  __syncthreads();
  const float c = c_sh;
  for (int t = lo + threadIdx.x; t < hi; t += blockDim.x) {
    float r = 1.f;
    if (lars && !excluded[t]) {
      const float wn = sqrtf(sq[t]);
      const float gn = sqrtf(sq[n + t]);
      if (wn > 0.f && gn > 0.f) r = eta * wn / (c * gn + wd * wn + LARS_EPS);
    }
    ratio[t] = r;
  }
}

// ---------------------------------------------------------------------------
// Multi-tensor unscale + inf/nan check (fp16 loss-scaler backward pass).
// ---------------------------------------------------------------------------
struct MTGradList {
  float* g[MT_MAX_TENSORS];
  int size[MT_MAX_TENSORS];
  int ntensors;
};

__global__ void multi_tensor_unscale_kernel(MTGradList tl, float inv_scale,
                                            int* __restrict__ found_inf) {
  int t, start, end;
  if (!mt_locate(tl, t, start, end)) return;
  float* g = tl.g[t];
  bool bad = false;
  for (int i = start + threadIdx.x; i < end; i += blockDim.x) {
    const float v = g[i] * inv_scale;
    g[i] = v;
    bad |= !isfinite(v);
  }
  if (__any(bad) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(found_inf, 1);
}

// ---------------------------------------------------------------------------
// Global average pool (AdaptiveAvgPool2d((1,1)), reference utils/model.py:76).
// NHWC: one thread per channel, strided over pixels (coalesced across lanes);
// NCHW: one block per (n,c) row, wave reduction.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void gap_fwd_nhwc_kernel(const scalar_t* __restrict__ x,
                                    scalar_t* __restrict__ y,
                                    int C, int S) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = blockIdx.y;
  if (c >= C) return;
  // 4 partial sums -> 4 loads in flight (the add chain otherwise
  // serialises one HBM-latency per pixel)
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const scalar_t* base = x + (long)n * S * C + c;
  int p = 0;
  for (; p + 4 <= S; p += 4) {
    s0 += (float)base[(long)p * C];
    s1 += (float)base[(long)(p + 1) * C];
    s2 += (float)base[(long)(p + 2) * C];
    s3 += (float)base[(long)(p + 3) * C];
  }
  for (; p < S; ++p) s0 += (float)base[(long)p * C];
  y[(long)n * C + c] = (scalar_t)((s0 + s1 + s2 + s3) / S);
}

template <typename scalar_t>
__global__ void gap_fwd_nchw_kernel(const scalar_t* __restrict__ x,
                                    scalar_t* __restrict__ y,
                                    int C, int S) {
  __shared__ float lds[32];
  const long row = blockIdx.x;  // n*C + c
  float s = 0.f;
  const scalar_t* base = x + row * S;
  for (int p = threadIdx.x; p < S; p += blockDim.x) s += (float)base[p];
  s = block_reduce_sum(s, lds);
  if (threadIdx.x == 0) y[row] = (scalar_t)(s / S);
}

template <typename scalar_t, bool CLAST>
__global__ void gap_bwd_kernel(const scalar_t* __restrict__ dy,
                               scalar_t* __restrict__ dx,
                               long total, int C, int S) {
  const float inv = 1.f / S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = CLAST ? i / ((long)S * C) : i / ((long)C * S);
    const int c = CLAST ? (int)(i % C) : (int)((i / S) % C);
    dx[i] = (scalar_t)((float)dy[n * C + c] * inv);
  }
}

// ---------------------------------------------------------------------------
// MaxPool2d NHWC (the ImageNet stem's 3x3 s2 pool). Forward records the
// window argmax (uint8, first-max tie-break like ATen); backward GATHERS:
// each input pixel sums the dy of the <=4 overlapping windows that chose
// it — no atomics, no scatter. Vectorized 16 B over channels.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void maxpool_fwd_nhwc_kernel(const scalar_t* __restrict__ x,
                                        scalar_t* __restrict__ y,
                                        unsigned char* __restrict__ idx,
                                        int Nb, int H, int W, int C,
                                        int P, int Q, int K, int S, int pad) {
  constexpr int V = 16 / sizeof(scalar_t);
  const long nvec = (long)Nb * P * Q * (C / V);
  const int cpr = C / V;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < nvec;
       o += (long)gridDim.x * blockDim.x) {
    const int cv = (int)(o % cpr);
    long t = o / cpr;
    const int q = (int)(t % Q); t /= Q;
    const int p = (int)(t % P);
    const int n = (int)(t / P);
    const int c0 = cv * V;
    float best[V];
    unsigned char bidx[V];
    #pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -3.4e38f; bidx[e] = 0; }
    const int ih0 = p * S - pad, iw0 = q * S - pad;
    for (int kh = 0; kh < K; ++kh) {
      const int ih = ih0 + kh;
      if (ih < 0 || ih >= H) continue;
      for (int kw = 0; kw < K; ++kw) {
        const int iw = iw0 + kw;
        if (iw < 0 || iw >= W) continue;
        scalar_t v[16 / sizeof(scalar_t)];
        *(float4*)v = *(const float4*)(x +
            (((long)n * H + ih) * W + iw) * C + c0);
        const unsigned char wi = (unsigned char)(kh * K + kw);
        #pragma unroll
        for (int e = 0; e < V; ++e) {
          const float f = (float)v[e];
          if (f > best[e]) { best[e] = f; bidx[e] = wi; }
        }
      }
    }
    scalar_t out[16 / sizeof(scalar_t)];
    #pragma unroll
    for (int e = 0; e < V; ++e) out[e] = (scalar_t)best[e];
    const long ob = (((long)n * P + p) * Q + q) * C + c0;
    *(float4*)(y + ob) = *(float4*)out;
    #pragma unroll
    for (int e = 0; e < V; ++e) idx[ob + e] = bidx[e];
  }
}

template <typename scalar_t>
__global__ void maxpool_bwd_nhwc_kernel(const scalar_t* __restrict__ dy,
                                        const unsigned char* __restrict__ idx,
                                        scalar_t* __restrict__ dx,
                                        int Nb, int H, int W, int C,
                                        int P, int Q, int K, int S, int pad) {
  constexpr int V = 16 / sizeof(scalar_t);
  const long nvec = (long)Nb * H * W * (C / V);
  const int cpr = C / V;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < nvec;
       o += (long)gridDim.x * blockDim.x) {
    const int cv = (int)(o % cpr);
    long t = o / cpr;
    const int iw = (int)(t % W); t /= W;
    const int ih = (int)(t % H);
    const int n = (int)(t / H);
    const int c0 = cv * V;
    float acc[V];
    #pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    // windows (p,q) with p*S - pad <= ih < p*S - pad + K
    const int p_lo = max(0, (ih + pad - K + S) / S);
    const int p_hi = min(P - 1, (ih + pad) / S);
    const int q_lo = max(0, (iw + pad - K + S) / S);
    const int q_hi = min(Q - 1, (iw + pad) / S);
    for (int p = p_lo; p <= p_hi; ++p) {
      const int kh = ih - (p * S - pad);
      if (kh < 0 || kh >= K) continue;
      for (int q = q_lo; q <= q_hi; ++q) {
        const int kw = iw - (q * S - pad);
        if (kw < 0 || kw >= K) continue;
        const long ob = (((long)n * P + p) * Q + q) * C + c0;
        const unsigned char wi = (unsigned char)(kh * K + kw);
        scalar_t g[16 / sizeof(scalar_t)];
        *(float4*)g = *(const float4*)(dy + ob);
        #pragma unroll
        for (int e = 0; e < V; ++e)
          if (idx[ob + e] == wi) acc[e] += (float)g[e];
      }
    }
    scalar_t out[16 / sizeof(scalar_t)];
    #pragma unroll
    for (int e = 0; e < V; ++e) out[e] = (scalar_t)acc[e];
    *(float4*)(dx + (((long)n * H + ih) * W + iw) * C + c0) = *(float4*)out;
  }
}

// ---------------------------------------------------------------------------
// Per-row rank of the target class:
//   rank = #{j : logit[j] > logit[t]} + #{j < t : logit[j] == logit[t]}.
// acc@k = mean(rank < k). Ties break by smaller class index (a stable
// descending sort's order — matches the reference's topk/eq pipeline,
// utils/util.py:50-64, including equal logits). One pass, no sort.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void class_rank_kernel(const scalar_t* __restrict__ logits,
                                  const long* __restrict__ target,
                                  int* __restrict__ rank, int N, int C) {
  __shared__ float lds[32];
  const int row = blockIdx.x;
  const scalar_t* xr = logits + (long)row * C;
  const int t = (int)target[row];
  const float tv = (float)xr[t];
  float cnt = 0.f;
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const float v = (float)xr[j];
    cnt += (v > tv || (v == tv && j < t)) ? 1.f : 0.f;
  }
  cnt = block_reduce_sum(cnt, lds);
  if (threadIdx.x == 0) rank[row] = (int)cnt;
}

int split_for(long per_channel_elems, int nchannels) {
  // enough blocks to fill 256 CUs even for small C
  long want = (2048 + nchannels - 1) / nchannels;
  long avail = (per_channel_elems + 255) / 256;
  int split = (int)std::max(1L, std::min(want, avail));
  return std::min(split, 64);
}

}  // namespace

// ===========================================================================
// Host-side launchers
// ===========================================================================

#define CHECK_CUDA(x) TORCH_CHECK(x.is_cuda(), #x " must be a HIP tensor")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

namespace {
inline bool is_clast(const at::Tensor& t) {
  return t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
         !t.is_contiguous();
}
inline void check_dense(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_contiguous() ||
              (t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast)),
              name, " must be NCHW- or NHWC-contiguous");
}
}  // namespace

std::vector<at::Tensor> bn_stats(at::Tensor x) {
  CHECK_CUDA(x); check_dense(x, "x");
  const int N = x.size(0), C = x.size(1);
  const long S = x.numel() / ((long)N * C);
  auto opts = x.options().dtype(at::kFloat);
  auto sum = at::zeros({C}, opts);
  auto sqsum = at::zeros({C}, opts);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_stats", [&] {
    if (is_clast(x)) {
      const long P = (long)N * S;
      const int cblocks = (C + 255) / 256;
      const int split = (int)std::min(P, (long)std::max(1, 768 / cblocks));
      hipLaunchKernelGGL(bn_stats_nhwc_kernel<scalar_t>, dim3(cblocks, split),
                         dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(), sum.data_ptr<float>(),
                         sqsum.data_ptr<float>(), P, C);
    } else {
      const int split = split_for((long)N * S, C);
      hipLaunchKernelGGL(bn_stats_kernel<scalar_t>, dim3(C, split), dim3(256),
                         0, cur_stream(),
                         x.data_ptr<scalar_t>(), sum.data_ptr<float>(),
                         sqsum.data_ptr<float>(), N, C, (int)S);
    }
  });
  return {sum, sqsum};
}

namespace {
// v2 NHWC kernels: each thread owns 8 consecutive channels, tpr = C/8
// threads per row, rpb = 256/tpr rows per iteration. Usable when C/8 is a
// power-of-two divisor of 256 (every ResNet18/50 BN width).
inline bool v2_ok(int C, int elem_size) {
  if (elem_size != 2 || C % 8 != 0) return false;
  const int tpr = C / 8;
  return tpr <= 256 && 256 % tpr == 0 && (tpr & (tpr - 1)) == 0;
}
inline int split_for_nhwc(long P, int rpb) {
  long want = 512;
  long avail = (P + rpb - 1) / rpb;
  return (int)std::min((long)512, std::min(want, avail));
}
inline bool takes_v2(const at::Tensor& x) {
  return is_clast(x) && v2_ok((int)x.size(1), (int)x.element_size());
}

// Half/BFloat16-only dispatch for the 16-byte-vector kernels.
template <typename F>
inline void dispatch_16bit(const at::Tensor& t, const char* name, F&& f) {
  if (t.scalar_type() == at::kBFloat16) f(at::BFloat16{});
  else if (t.scalar_type() == at::kHalf) f(at::Half{});
  else TORCH_CHECK(false, name, ": expected a Half or BFloat16 tensor");
}

// The v2 stats launch alone: per-block partial [split][2C], not yet reduced
// over split (bn_reduce_partials_kernel or a tail kernel does that).
at::Tensor stats_partial_v2(const at::Tensor& x) {
  const int C = x.size(1);
  const long P = x.numel() / C;
  const int tpr = C / 8, rpb = 256 / tpr;
  const int split = split_for_nhwc(P, rpb);
  auto partial = at::empty({split, 2L * C}, x.options().dtype(at::kFloat));
  dispatch_16bit(x, "bn_stats_partial", [&](auto tag) {
    using scalar_t = decltype(tag);
    hipLaunchKernelGGL(bn_stats_nhwc_v2_kernel<scalar_t>,
                       dim3(1, split), dim3(256), 0, cur_stream(),
                       x.data_ptr<scalar_t>(), partial.data_ptr<float>(),
                       P, C, tpr);
  });
  return partial;
}

at::Tensor bwd_reduce_partial_v2(const at::Tensor& dy, const at::Tensor& x,
                                 const at::Tensor& mean,
                                 const at::Tensor& invstd,
                                 const at::Tensor& y, bool relu) {
  const int C = x.size(1);
  const long P = x.numel() / C;
  const int tpr = C / 8, rpb = 256 / tpr;
  const int split = split_for_nhwc(P, rpb);
  auto partial = at::empty({split, 2L * C}, x.options().dtype(at::kFloat));
  dispatch_16bit(x, "bn_bwd_reduce_partial", [&](auto tag) {
    using scalar_t = decltype(tag);
    auto launch = [&](auto relu_c) {
      hipLaunchKernelGGL((bn_bwd_reduce_nhwc_v2_kernel<scalar_t,
                                                       decltype(relu_c)::value>),
                         dim3(1, split), dim3(256), 0, cur_stream(),
                         dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                         y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), partial.data_ptr<float>(),
                         P, C, tpr);
    };
    relu ? launch(std::true_type{}) : launch(std::false_type{});
  });
  return partial;
}

at::Tensor reduce_partials(const at::Tensor& partial) {
  const int split = partial.size(0);
  const long twoC = partial.size(1);
  auto packed = at::empty({twoC}, partial.options());
  hipLaunchKernelGGL(bn_reduce_partials_kernel,
                     dim3((int)twoC), dim3(256), 0, cur_stream(),
                     partial.data_ptr<float>(), packed.data_ptr<float>(),
                     split, (int)twoC);
  return packed;
}
}  // namespace

// True when x takes the NHWC v2 stats/reduce kernels, i.e. when
// bn_stats_partial / bn_bwd_reduce_partial and the tail kernels apply.
bool bn_v2_ok(at::Tensor x) {
  return x.is_cuda() && x.dim() == 4 && takes_v2(x);
}

// Per-block {sum, sqsum} partial [split][2C] of the v2 path, unreduced:
// bn_fwd_tail folds it. bn_stats_packed(x) is this plus the reduce launch.
at::Tensor bn_stats_partial(at::Tensor x) {
  CHECK_CUDA(x); check_dense(x, "x");
  TORCH_CHECK(takes_v2(x), "bn_stats_partial: x must take the NHWC v2 path "
              "(see bn_v2_ok)");
  return stats_partial_v2(x);
}

// Per-channel {sum, sqsum} packed into ONE [2C] fp32 tensor (the layout the
// SyncBN all_reduce and bn_finalize consume).
at::Tensor bn_stats_packed(at::Tensor x) {
  CHECK_CUDA(x); check_dense(x, "x");
  const int N = x.size(0), C = x.size(1);
  const long S = x.numel() / ((long)N * C);
  auto opts = x.options().dtype(at::kFloat);
  at::Tensor result;
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_stats_packed", [&] {
    if (is_clast(x) && v2_ok(C, (int)sizeof(scalar_t))) {
      result = reduce_partials(stats_partial_v2(x));
    } else if (is_clast(x)) {
      const long P = (long)N * S;
      auto packed = at::zeros({2L * C}, opts);
      const int cblocks = (C + 255) / 256;
      const int split = (int)std::min(P, (long)std::max(1, 768 / cblocks));
      hipLaunchKernelGGL(bn_stats_nhwc_kernel<scalar_t>, dim3(cblocks, split),
                         dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(), packed.data_ptr<float>(),
                         packed.data_ptr<float>() + C, P, C);
      result = packed;
    } else {
      auto packed = at::zeros({2L * C}, opts);
      const int split = split_for((long)N * S, C);
      hipLaunchKernelGGL(bn_stats_kernel<scalar_t>, dim3(C, split), dim3(256),
                         0, cur_stream(),
                         x.data_ptr<scalar_t>(), packed.data_ptr<float>(),
                         packed.data_ptr<float>() + C, N, C, (int)S);
      result = packed;
    }
  });
  return result;
}

// packed {sum,sqsum} -> (mean, invstd); updates running stats in-place when
// given. One launch replaces the eager mean/var/clamp/rsqrt/lerp chain.
std::vector<at::Tensor> bn_finalize(at::Tensor packed, double count,
                                    double momentum, double eps,
                                    c10::optional<at::Tensor> running_mean,
                                    c10::optional<at::Tensor> running_var) {
  CHECK_CUDA(packed); CHECK_CONTIG(packed);
  const int C = packed.numel() / 2;
  auto mean = at::empty({C}, packed.options());
  auto invstd = at::empty({C}, packed.options());
  float* rm = running_mean ? running_mean->data_ptr<float>() : nullptr;
  float* rv = running_var ? running_var->data_ptr<float>() : nullptr;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0,
                     cur_stream(), packed.data_ptr<float>(),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(), rm, rv,
                     (float)count, (float)momentum, (float)eps, C);
  return {mean, invstd};
}

namespace {
// partial is [split][2C], or a packed [2C] (split = 1)
inline void check_partial(const at::Tensor& partial, int* split, int* C) {
  CHECK_CUDA(partial); CHECK_CONTIG(partial);
  TORCH_CHECK(partial.scalar_type() == at::kFloat &&
              (partial.dim() == 1 || partial.dim() == 2) &&
              partial.size(-1) % 2 == 0,
              "partial must be fp32 [split][2C] or [2C]");
  *split = partial.dim() == 2 ? (int)partial.size(0) : 1;
  *C = (int)(partial.size(-1) / 2);
}
inline const float* chan_ptr(const at::Tensor& t, int C, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kFloat && t.numel() == C,
              name, " must be a contiguous fp32 HIP tensor of C elements");
  return t.data_ptr<float>();
}
}  // namespace

// partial {sum,sqsum} [split][2C] (or packed [2C]) -> {stats, mean, invstd}:
// stats is fp32 [4][C] = {mean, invstd, scale, shift} for bn_fwd_apply; mean
// and invstd are its first two rows as views. Updates running stats in
// place when given. One launch: reduce + finalize + coefficient fold.
std::vector<at::Tensor> bn_fwd_tail(at::Tensor partial, at::Tensor weight,
                                    at::Tensor bias, double count,
                                    double momentum, double eps,
                                    c10::optional<at::Tensor> running_mean,
                                    c10::optional<at::Tensor> running_var) {
  int split, C;
  check_partial(partial, &split, &C);
  const float* w = chan_ptr(weight, C, "weight");
  const float* b = chan_ptr(bias, C, "bias");
  TORCH_CHECK(running_mean.has_value() == running_var.has_value(),
              "running_mean and running_var go together");
  float* rm = running_mean ?
      const_cast<float*>(chan_ptr(*running_mean, C, "running_mean")) : nullptr;
  float* rv = running_var ?
      const_cast<float*>(chan_ptr(*running_var, C, "running_var")) : nullptr;
  auto stats = at::empty({4, C}, partial.options());
  hipLaunchKernelGGL(bn_fwd_tail_kernel, dim3(C), dim3(256), 0, cur_stream(),
                     partial.data_ptr<float>(), w, b, stats.data_ptr<float>(),
                     rm, rv, (float)count, (float)momentum, (float)eps,
                     split, C);
  return {stats, stats.select(0, 0), stats.select(0, 1)};
}

// {sum_dy, sum_dy_xhat} packed [2C], relu mask folded in.
at::Tensor bn_bwd_reduce_packed(at::Tensor dy, at::Tensor x, at::Tensor mean,
                                at::Tensor invstd, at::Tensor y, bool relu) {
  CHECK_CUDA(dy); check_dense(dy, "dy"); check_dense(x, "x");
  TORCH_CHECK(is_clast(dy) == is_clast(x), "dy/x layout mismatch");
  const int N = x.size(0), C = x.size(1);
  const long S = x.numel() / ((long)N * C);
  auto opts = x.options().dtype(at::kFloat);
  at::Tensor result;
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_bwd_reduce_packed", [&] {
    if (is_clast(x) && v2_ok(C, (int)sizeof(scalar_t))) {
      result = reduce_partials(
          bwd_reduce_partial_v2(dy, x, mean, invstd, y, relu));
    } else if (is_clast(x)) {
      const long P = (long)N * S;
      auto packed = at::zeros({2L * C}, opts);
      const int cblocks = (C + 255) / 256;
      const int split = (int)std::min(P, (long)std::max(1, 768 / cblocks));
      auto launch = [&](auto relu_c) {
        hipLaunchKernelGGL((bn_bwd_reduce_nhwc_kernel<scalar_t,
                                                      decltype(relu_c)::value>),
                           dim3(cblocks, split), dim3(256), 0, cur_stream(),
                           dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                           y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), packed.data_ptr<float>(),
                           packed.data_ptr<float>() + C, P, C);
      };
      relu ? launch(std::true_type{}) : launch(std::false_type{});
      result = packed;
    } else {
      auto packed = at::zeros({2L * C}, opts);
      const int split = split_for((long)N * S, C);
      auto launch = [&](auto relu_c) {
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<scalar_t,
                                                 decltype(relu_c)::value>),
                           dim3(C, split), dim3(256), 0, cur_stream(),
                           dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                           y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), packed.data_ptr<float>(),
                           packed.data_ptr<float>() + C, N, C, (int)S);
      };
      relu ? launch(std::true_type{}) : launch(std::false_type{});
      result = packed;
    }
  });
  return result;
}

// Per-block {sum_dy, sum_dy_xhat} partial [split][2C] of the v2 path,
// unreduced: bn_bwd_tail folds it. bn_bwd_reduce_packed is this plus the
// reduce launch.
at::Tensor bn_bwd_reduce_partial(at::Tensor dy, at::Tensor x, at::Tensor mean,
                                 at::Tensor invstd, at::Tensor y, bool relu) {
  CHECK_CUDA(dy); check_dense(dy, "dy"); check_dense(x, "x");
  TORCH_CHECK(takes_v2(x), "bn_bwd_reduce_partial: x must take the NHWC v2 "
              "path (see bn_v2_ok)");
  TORCH_CHECK(is_clast(dy) && dy.sizes() == x.sizes() &&
              dy.scalar_type() == x.scalar_type(), "dy/x mismatch");
  if (relu) {
    TORCH_CHECK(is_clast(y) && y.sizes() == x.sizes() &&
                y.scalar_type() == x.scalar_type(), "y/x mismatch");
  }
  const int C = x.size(1);
  chan_ptr(mean, C, "mean");
  chan_ptr(invstd, C, "invstd");
  return bwd_reduce_partial_v2(dy, x, mean, invstd, y, relu);
}

// partial [split][2C] -> {dbeta, dgamma, coeffs}: dbeta = sum_dy and dgamma =
// sum_dy_xhat are the two rows of one fresh fp32 [2][C] tensor (views, no
// copy); coeffs is fp32 [3][C] = {A, B, D} for bn_bwd_apply. One launch:
// reduce + backward coefficient fold.
std::vector<at::Tensor> bn_bwd_tail(at::Tensor partial, at::Tensor weight,
                                    at::Tensor mean, at::Tensor invstd,
                                    double inv_count, bool training) {
  int split, C;
  check_partial(partial, &split, &C);
  const float* w = chan_ptr(weight, C, "weight");
  const float* mu = chan_ptr(mean, C, "mean");
  const float* is = chan_ptr(invstd, C, "invstd");
  auto sums = at::empty({2, C}, partial.options());
  auto coeffs = at::empty({3, C}, partial.options());
  hipLaunchKernelGGL(bn_bwd_tail_kernel<false>, dim3(C), dim3(256), 0,
                     cur_stream(), partial.data_ptr<float>(), w, mu, is,
                     (float)inv_count, training, sums.data_ptr<float>(),
                     coeffs.data_ptr<float>(), split, C);
  return {sums.select(0, 0), sums.select(0, 1), coeffs};
}

// SyncBN variant: no coefficients (they need the cross-rank sums); the sums
// are written twice instead, {dbeta, dgamma} rows for the local grads and
// packed [2C] for the all_reduce to overwrite.
std::vector<at::Tensor> bn_bwd_tail_dup(at::Tensor partial) {
  int split, C;
  check_partial(partial, &split, &C);
  auto sums = at::empty({2, C}, partial.options());
  auto packed = at::empty({2L * C}, partial.options());
  hipLaunchKernelGGL(bn_bwd_tail_kernel<true>, dim3(C), dim3(256), 0,
                     cur_stream(), partial.data_ptr<float>(), nullptr, nullptr,
                     nullptr, 0.f, false, sums.data_ptr<float>(),
                     packed.data_ptr<float>(), split, C);
  return {sums.select(0, 0), sums.select(0, 1), packed};
}

namespace {
// y = x*scale[c] + shift[c] (+res)(relu): the bn_fwd_vec_kernel launch alone.
void launch_bn_fwd_vec(const at::Tensor& x, const at::Tensor& residual,
                       bool has_res, at::Tensor& y, const float* sc,
                       const float* sh, bool relu) {
  const int N = x.size(0), C = x.size(1);
  const int S = x.numel() / ((long)N * C);
  const bool clast = is_clast(x);
  const long nvec = x.numel() / 8;
  const int vblocks = (int)std::min((nvec + 255) / 256, (long)2048);
  dispatch_16bit(x, "bn_fwd", [&](auto tag) {
    using scalar_t = decltype(tag);
    auto launch = [&](auto relu_c, auto res_c, auto cl_c) {
      hipLaunchKernelGGL((bn_fwd_vec_kernel<scalar_t, decltype(relu_c)::value,
                                            decltype(res_c)::value,
                                            decltype(cl_c)::value>),
                         dim3(vblocks), dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(),
                         has_res ? residual.data_ptr<scalar_t>() : nullptr,
                         y.data_ptr<scalar_t>(), sc, sh, nvec, C, S);
    };
    auto l2 = [&](auto relu_c, auto res_c) {
      clast ? launch(relu_c, res_c, std::true_type{})
            : launch(relu_c, res_c, std::false_type{});
    };
    if (relu && has_res) l2(std::true_type{}, std::true_type{});
    else if (relu) l2(std::true_type{}, std::false_type{});
    else if (has_res) l2(std::false_type{}, std::true_type{});
    else l2(std::false_type{}, std::false_type{});
  });
}
inline bool bn_vec_ok(const at::Tensor& x) {
  const int N = x.size(0), C = x.size(1);
  const long S = x.numel() / ((long)N * C);
  return x.element_size() == 2 && x.numel() % 8 == 0 &&
         (is_clast(x) ? (C % 8 == 0) : (S % 8 == 0));
}
}  // namespace

// Forward apply from precomputed coefficients: stats is bn_fwd_tail's fp32
// [4][C] (rows 2, 3 = scale, shift). Launches only bn_fwd_vec_kernel.
at::Tensor bn_fwd_apply(at::Tensor x, at::Tensor stats, bool relu,
                        c10::optional<at::Tensor> residual_opt) {
  const at::Tensor residual = residual_opt ? *residual_opt : at::Tensor();
  CHECK_CUDA(x); check_dense(x, "x");
  TORCH_CHECK(x.dim() == 4 && bn_vec_ok(x),
              "bn_fwd_apply: x must take the vectorised path");
  const int C = x.size(1);
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() &&
              stats.scalar_type() == at::kFloat && stats.dim() == 2 &&
              stats.size(0) == 4 && stats.size(1) == C,
              "stats must be fp32 [4][C]");
  const bool has_res = residual.defined() && residual.numel() > 0;
  if (has_res) {
    TORCH_CHECK(is_clast(residual) == is_clast(x) &&
                residual.sizes() == x.sizes() &&
                residual.scalar_type() == x.scalar_type(),
                "residual layout mismatch");
  }
  auto y = at::empty_like(x);
  const float* sc = stats.data_ptr<float>() + 2L * C;
  launch_bn_fwd_vec(x, residual, has_res, y, sc, sc + C, relu);
  return y;
}

at::Tensor bn_fwd(at::Tensor x, at::Tensor weight, at::Tensor bias,
                  at::Tensor mean, at::Tensor invstd, bool relu,
                  at::Tensor residual) {
  CHECK_CUDA(x); check_dense(x, "x");
  const int N = x.size(0), C = x.size(1);
  const int S = x.numel() / ((long)N * C);
  const long total = x.numel();
  const bool has_res = residual.defined() && residual.numel() > 0;
  const bool clast = is_clast(x);
  if (has_res) {
    TORCH_CHECK(is_clast(residual) == clast, "residual layout mismatch");
  }
  auto y = at::empty_like(x);
  auto wf = weight.to(at::kFloat).contiguous();
  auto bf = bias.to(at::kFloat).contiguous();
  const int blocks = (int)std::min((total + 1023) / 1024, (long)4096);
  if (bn_vec_ok(x)) {
    auto coeffs = at::empty({2, C}, x.options().dtype(at::kFloat));
    float* sc = coeffs.data_ptr<float>();
    float* sh = sc + C;
    hipLaunchKernelGGL(bn_coeffs_kernel, dim3((C + 255) / 256), dim3(256),
                       0, cur_stream(), wf.data_ptr<float>(),
                       bf.data_ptr<float>(), mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), sc, sh, C);
    launch_bn_fwd_vec(x, residual, has_res, y, sc, sh, relu);
    return y;
  }
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_fwd", [&] {
    auto launch = [&](auto relu_c, auto res_c, auto cl_c) {
      hipLaunchKernelGGL((bn_fwd_kernel<scalar_t, decltype(relu_c)::value,
                                        decltype(res_c)::value,
                                        decltype(cl_c)::value>),
                         dim3(blocks), dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(),
                         has_res ? residual.data_ptr<scalar_t>() : nullptr,
                         y.data_ptr<scalar_t>(), wf.data_ptr<float>(),
                         bf.data_ptr<float>(), mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), total, C, S);
    };
    auto l2 = [&](auto relu_c, auto res_c) {
      clast ? launch(relu_c, res_c, std::true_type{})
            : launch(relu_c, res_c, std::false_type{});
    };
    if (relu && has_res) l2(std::true_type{}, std::true_type{});
    else if (relu) l2(std::true_type{}, std::false_type{});
    else if (has_res) l2(std::false_type{}, std::true_type{});
    else l2(std::false_type{}, std::false_type{});
  });
  return y;
}

std::vector<at::Tensor> bn_bwd_reduce(at::Tensor dy, at::Tensor x,
                                      at::Tensor mean, at::Tensor invstd,
                                      at::Tensor y, bool relu) {
  CHECK_CUDA(dy); check_dense(dy, "dy"); check_dense(x, "x");
  TORCH_CHECK(is_clast(dy) == is_clast(x), "dy/x layout mismatch");
  const int N = x.size(0), C = x.size(1);
  const long S = x.numel() / ((long)N * C);
  auto opts = x.options().dtype(at::kFloat);
  auto sum_dy = at::zeros({C}, opts);
  auto sum_dy_xhat = at::zeros({C}, opts);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_bwd_reduce", [&] {
    if (is_clast(x)) {
      const long P = (long)N * S;
      const int cblocks = (C + 255) / 256;
      const int split = (int)std::min(P, (long)std::max(1, 768 / cblocks));
      auto launch = [&](auto relu_c) {
        hipLaunchKernelGGL((bn_bwd_reduce_nhwc_kernel<scalar_t,
                                                      decltype(relu_c)::value>),
                           dim3(cblocks, split), dim3(256), 0, cur_stream(),
                           dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                           y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), sum_dy.data_ptr<float>(),
                           sum_dy_xhat.data_ptr<float>(), P, C);
      };
      relu ? launch(std::true_type{}) : launch(std::false_type{});
    } else {
      const int split = split_for((long)N * S, C);
      auto launch = [&](auto relu_c) {
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<scalar_t,
                                                 decltype(relu_c)::value>),
                           dim3(C, split), dim3(256), 0, cur_stream(),
                           dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                           y.data_ptr<scalar_t>(), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), sum_dy.data_ptr<float>(),
                           sum_dy_xhat.data_ptr<float>(), N, C, (int)S);
      };
      relu ? launch(std::true_type{}) : launch(std::false_type{});
    }
  });
  return {sum_dy, sum_dy_xhat};
}

namespace {
// dx = A*g + B*x + D (+ dres): the bn_bwd_vec_kernel launch alone. A points
// at the contiguous [3][C] {A, B, D} table.
void launch_bn_bwd_vec(const at::Tensor& dy, const at::Tensor& x,
                       const at::Tensor& y, at::Tensor& dx, at::Tensor& dres,
                       const float* A, bool relu, bool training,
                       bool need_dres) {
  const int N = x.size(0), C = x.size(1);
  const int S = x.numel() / ((long)N * C);
  const bool clast = is_clast(x);
  const float* B = A + C;
  const float* D = B + C;
  const long nvec = x.numel() / 8;
  const int vblocks = (int)std::min((nvec + 255) / 256, (long)2048);
  dispatch_16bit(x, "bn_bwd", [&](auto tag) {
    using scalar_t = decltype(tag);
    auto launch = [&](auto relu_c, auto train_c, auto dres_c, auto cl_c) {
      hipLaunchKernelGGL((bn_bwd_vec_kernel<scalar_t, decltype(relu_c)::value,
                                            decltype(train_c)::value,
                                            decltype(dres_c)::value,
                                            decltype(cl_c)::value>),
                         dim3(vblocks), dim3(256), 0, cur_stream(),
                         dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                         y.data_ptr<scalar_t>(), dx.data_ptr<scalar_t>(),
                         need_dres ? dres.data_ptr<scalar_t>() : nullptr,
                         A, B, D, nvec, C, S);
    };
    auto l3 = [&](auto relu_c, auto train_c, auto dres_c) {
      clast ? launch(relu_c, train_c, dres_c, std::true_type{})
            : launch(relu_c, train_c, dres_c, std::false_type{});
    };
    auto l2 = [&](auto relu_c, auto train_c) {
      need_dres ? l3(relu_c, train_c, std::true_type{})
                : l3(relu_c, train_c, std::false_type{});
    };
    if (relu) {
      training ? l2(std::true_type{}, std::true_type{})
               : l2(std::true_type{}, std::false_type{});
    } else {
      training ? l2(std::false_type{}, std::true_type{})
               : l2(std::false_type{}, std::false_type{});
    }
  });
}
}  // namespace

// Backward apply from precomputed coefficients: coeffs is bn_bwd_tail's fp32
// [3][C] = {A, B, D}. Launches only bn_bwd_vec_kernel. Returns {dx, dres}.
std::vector<at::Tensor> bn_bwd_apply(at::Tensor dy, at::Tensor x, at::Tensor y,
                                     at::Tensor coeffs, bool relu,
                                     bool training, bool need_dres) {
  CHECK_CUDA(dy); check_dense(dy, "dy"); check_dense(x, "x");
  TORCH_CHECK(x.dim() == 4 && bn_vec_ok(x),
              "bn_bwd_apply: x must take the vectorised path");
  TORCH_CHECK(is_clast(dy) == is_clast(x) && dy.sizes() == x.sizes() &&
              dy.scalar_type() == x.scalar_type(), "dy/x mismatch");
  if (relu) {
    TORCH_CHECK(is_clast(y) == is_clast(x) && y.sizes() == x.sizes() &&
                y.scalar_type() == x.scalar_type(), "y/x mismatch");
  }
  const int C = x.size(1);
  TORCH_CHECK(coeffs.is_cuda() && coeffs.is_contiguous() &&
              coeffs.scalar_type() == at::kFloat && coeffs.dim() == 2 &&
              coeffs.size(0) == 3 && coeffs.size(1) == C,
              "coeffs must be fp32 [3][C]");
  auto dx = at::empty_like(x);
  auto dres = need_dres ? at::empty_like(x) : at::empty({0}, x.options());
  launch_bn_bwd_vec(dy, x, y, dx, dres, coeffs.data_ptr<float>(), relu,
                    training, need_dres);
  return {dx, dres};
}

std::vector<at::Tensor> bn_bwd(at::Tensor dy, at::Tensor x, at::Tensor weight,
                               at::Tensor mean, at::Tensor invstd,
                               at::Tensor sum_dy, at::Tensor sum_dy_xhat,
                               double count, at::Tensor y, bool relu,
                               bool training, bool need_dres) {
  CHECK_CUDA(dy); check_dense(dy, "dy"); check_dense(x, "x");
  const int N = x.size(0), C = x.size(1);
  const int S = x.numel() / ((long)N * C);
  const long total = x.numel();
  const bool clast = is_clast(x);
  auto dx = at::empty_like(x);
  auto dres = need_dres ? at::empty_like(x) : at::empty({0}, x.options());
  auto wf = weight.to(at::kFloat).contiguous();
  const int blocks = (int)std::min((total + 1023) / 1024, (long)4096);
  if (bn_vec_ok(x)) {
    auto coeffs = at::empty({3, C}, x.options().dtype(at::kFloat));
    float* A = coeffs.data_ptr<float>();
    float* B = A + C;
    float* D = B + C;
    hipLaunchKernelGGL(bn_bwd_coeffs_kernel, dim3((C + 255) / 256),
                       dim3(256), 0, cur_stream(), wf.data_ptr<float>(),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       sum_dy.data_ptr<float>(),
                       sum_dy_xhat.data_ptr<float>(),
                       (float)(1.0 / count), training, A, B, D, C);
    launch_bn_bwd_vec(dy, x, y, dx, dres, A, relu, training, need_dres);
    return {dx, dres};
  }
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "bn_bwd", [&] {
    auto launch = [&](auto relu_c, auto train_c, auto dres_c, auto cl_c) {
      hipLaunchKernelGGL((bn_bwd_kernel<scalar_t, decltype(relu_c)::value,
                                        decltype(train_c)::value,
                                        decltype(dres_c)::value,
                                        decltype(cl_c)::value>),
                         dim3(blocks), dim3(256), 0, cur_stream(),
                         dy.data_ptr<scalar_t>(), x.data_ptr<scalar_t>(),
                         y.data_ptr<scalar_t>(), dx.data_ptr<scalar_t>(),
                         need_dres ? dres.data_ptr<scalar_t>() : nullptr,
                         wf.data_ptr<float>(), mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), sum_dy.data_ptr<float>(),
                         sum_dy_xhat.data_ptr<float>(),
                         (float)(1.0 / count), total, C, S);
    };
    auto l3 = [&](auto relu_c, auto train_c, auto dres_c) {
      clast ? launch(relu_c, train_c, dres_c, std::true_type{})
            : launch(relu_c, train_c, dres_c, std::false_type{});
    };
    if (relu) {
      if (training) need_dres ? l3(std::true_type{}, std::true_type{}, std::true_type{})
                              : l3(std::true_type{}, std::true_type{}, std::false_type{});
      else need_dres ? l3(std::true_type{}, std::false_type{}, std::true_type{})
                     : l3(std::true_type{}, std::false_type{}, std::false_type{});
    } else {
      if (training) need_dres ? l3(std::false_type{}, std::true_type{}, std::true_type{})
                              : l3(std::false_type{}, std::true_type{}, std::false_type{});
      else need_dres ? l3(std::false_type{}, std::false_type{}, std::true_type{})
                     : l3(std::false_type{}, std::false_type{}, std::false_type{});
    }
  });
  return {dx, dres};
}

std::vector<at::Tensor> xent_fwd(at::Tensor logits, at::Tensor target) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  TORCH_CHECK(target.scalar_type() == at::kLong, "target must be int64");
  const int N = logits.size(0), C = logits.size(1);
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  auto row_loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto loss = at::empty({}, logits.options().dtype(at::kFloat));
  const int threads = C <= 128 ? 64 : 256;
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      logits.scalar_type(), "xent_fwd", [&] {
    hipLaunchKernelGGL(xent_fwd_kernel<scalar_t>, dim3(N), dim3(threads), 0,
                       cur_stream(),
                       logits.data_ptr<scalar_t>(), target.data_ptr<long>(),
                       lse.data_ptr<float>(), row_loss.data_ptr<float>(), N, C);
  });
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     row_loss.data_ptr<float>(), loss.data_ptr<float>(), N);
  return {loss, lse};
}

at::Tensor xent_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                    at::Tensor dloss) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  const int N = logits.size(0), C = logits.size(1);
  const long total = logits.numel();
  auto dx = at::empty_like(logits);
  auto dloss_f = dloss.to(at::kFloat).contiguous();
  const int blocks = (int)std::min((total + 255) / 256, (long)4096);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      logits.scalar_type(), "xent_bwd", [&] {
    hipLaunchKernelGGL(xent_bwd_kernel<scalar_t>, dim3(blocks), dim3(256), 0,
                       cur_stream(),
                       logits.data_ptr<scalar_t>(), target.data_ptr<long>(),
                       lse.data_ptr<float>(), dloss_f.data_ptr<float>(),
                       dx.data_ptr<scalar_t>(), total, C);
  });
  return dx;
}

static void check_mix_targets(const at::Tensor& logits, const at::Tensor& ta,
                              const at::Tensor& tb, const at::Tensor& lam,
                              double eps) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1,
              "logits must be a non-empty [N, C] tensor");
  const long N = logits.size(0);
  const auto dev = logits.device();
  TORCH_CHECK(ta.scalar_type() == at::kLong && tb.scalar_type() == at::kLong,
              "target_a and target_b must be int64");
  TORCH_CHECK(lam.scalar_type() == at::kFloat, "lam must be float32");
  TORCH_CHECK(ta.device() == dev && tb.device() == dev && lam.device() == dev,
              "target_a, target_b and lam must be on the logits' device");
  TORCH_CHECK(ta.dim() == 1 && ta.size(0) == N && ta.is_contiguous() &&
              tb.dim() == 1 && tb.size(0) == N && tb.is_contiguous() &&
              lam.dim() == 1 && lam.size(0) == N && lam.is_contiguous(),
              "target_a, target_b and lam must be contiguous [N] tensors");
  TORCH_CHECK(eps >= 0.0 && eps < 1.0, "label smoothing must be in [0, 1)");
}

std::vector<at::Tensor> xent_mix_fwd(at::Tensor logits, at::Tensor target_a,
                                     at::Tensor target_b, at::Tensor lam,
                                     double eps) {
  check_mix_targets(logits, target_a, target_b, lam, eps);
  const int N = logits.size(0), C = logits.size(1);
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  auto row_loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto loss = at::empty({}, logits.options().dtype(at::kFloat));
  const int threads = C <= 128 ? 64 : 256;
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      logits.scalar_type(), "xent_mix_fwd", [&] {
    hipLaunchKernelGGL(xent_mix_fwd_kernel<scalar_t>, dim3(N), dim3(threads),
                       0, cur_stream(),
                       logits.data_ptr<scalar_t>(), target_a.data_ptr<long>(),
                       target_b.data_ptr<long>(), lam.data_ptr<float>(),
                       lse.data_ptr<float>(), row_loss.data_ptr<float>(),
                       (float)eps, N, C);
  });
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     row_loss.data_ptr<float>(), loss.data_ptr<float>(), N);
  return {loss, lse};
}

at::Tensor xent_mix_bwd(at::Tensor logits, at::Tensor target_a,
                        at::Tensor target_b, at::Tensor lam, at::Tensor lse,
                        at::Tensor dloss, double eps) {
  check_mix_targets(logits, target_a, target_b, lam, eps);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.numel() == logits.size(0) && lse.device() == logits.device(),
              "lse must be the contiguous float32 [N] tensor of xent_mix_fwd");
  const int C = logits.size(1);
  const long total = logits.numel();
  auto dx = at::empty_like(logits);
  auto dloss_f = dloss.to(at::kFloat).contiguous();
  const int blocks = (int)std::min((total + 255) / 256, (long)4096);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      logits.scalar_type(), "xent_mix_bwd", [&] {
    hipLaunchKernelGGL(xent_mix_bwd_kernel<scalar_t>, dim3(blocks), dim3(256),
                       0, cur_stream(),
                       logits.data_ptr<scalar_t>(), target_a.data_ptr<long>(),
                       target_b.data_ptr<long>(), lam.data_ptr<float>(),
                       lse.data_ptr<float>(), dloss_f.data_ptr<float>(),
                       dx.data_ptr<scalar_t>(), (float)eps, total, C);
  });
  return dx;
}

// One launch of a multi-tensor kernel in the making. The batching rule lives
// here and in mt_chunks only: at most MT_MAX_TENSORS tensors per launch,
// mt_chunks(numel) blocks per tensor.
template <typename List>
struct MTBatch {
  List tl;
  int nblocks = 0;
  MTBatch() { tl.ntensors = 0; }
  bool full() const { return tl.ntensors == MT_MAX_TENSORS; }
  // Takes a tensor of numel elements; returns its slot in tl.
  int push(int64_t numel) {
    const int t = tl.ntensors++;
    tl.size[t] = (int)numel;
    nblocks += mt_chunks(tl.size[t]);
    return t;
  }
};

typedef std::vector<c10::optional<at::Tensor>> OptTensors;

// emas[i], where given, as float* for the list structs: fp32 in the layout of
// `like` (the fp32 parameter or the O2 master), else null.
static float* ema_ptr(const OptTensors& emas, size_t i, const at::Tensor& like,
                      const char* who) {
  if (emas.empty() || !emas[i].has_value()) return nullptr;
  const at::Tensor& e = *emas[i];
  TORCH_CHECK(e.is_cuda() && e.device() == like.device() &&
              e.scalar_type() == at::kFloat && e.numel() == like.numel() &&
              e.sizes() == like.sizes() && e.strides() == like.strides(),
              who, ": ema must be float32 in the weight's layout");
  return e.data_ptr<float>();
}

// The two floats every EMA kernel takes: d and 1 - d, formed once here.
struct EmaDecay {
  float d, omd;
  explicit EmaDecay(double decay) : d((float)decay), omd(1.f - (float)decay) {
    TORCH_CHECK(decay >= 0 && decay <= 1, "ema_decay must be in [0, 1], got ",
                decay);
  }
};

// gscale/ratio null: the plain kernel. Otherwise the scaled one, with
// ratio[i] the coefficient of params[i]. emas empty: no averages, and the
// kernels launched are the ones without EMA.
static void multi_tensor_sgd_impl(std::vector<at::Tensor>& params,
                                  std::vector<at::Tensor>& grads,
                                  std::vector<at::Tensor>& bufs,
                                  double lr, double momentum,
                                  double weight_decay,
                                  std::vector<c10::optional<at::Tensor>>& w16s,
                                  const float* gscale, const float* ratio,
                                  const OptTensors& emas, double ema_decay) {
  const bool has_momentum = !bufs.empty();
  const bool scaled = gscale != nullptr;
  const bool ema = !emas.empty();
  const EmaDecay dec(ema_decay);
  TORCH_CHECK(params.size() == grads.size());
  TORCH_CHECK(!ema || emas.size() == params.size(),
              "multi_tensor_sgd: one ema entry (or None) per param");
  TORCH_CHECK(!has_momentum || bufs.size() == params.size(),
              "multi_tensor_sgd: one momentum buffer per param");
  TORCH_CHECK(w16s.empty() || w16s.size() == params.size(),
              "multi_tensor_sgd: one w16 entry (or None) per param");
  auto stream = cur_stream();
  for (size_t i = 0; i < params.size();) {
    MTBatch<MTTensorList> b;
    MTTensorList& tl = b.tl;
    const size_t first = i;
    for (; !b.full() && i < params.size(); ++i) {
      auto& p = params[i];
      TORCH_CHECK(p.is_cuda() && p.is_non_overlapping_and_dense() &&
                  p.scalar_type() == at::kFloat,
                  "multi_tensor_sgd expects dense fp32 params");
      TORCH_CHECK(grads[i].strides() == p.strides(),
                  "multi_tensor_sgd: grad/param layout mismatch");
      const int t = b.push(p.numel());
      tl.p[t] = p.data_ptr<float>();
      tl.g[t] = grads[i].data_ptr<float>();
      tl.m[t] = has_momentum ? bufs[i].data_ptr<float>() : nullptr;
      tl.ema[t] = ema_ptr(emas, i, p, "multi_tensor_sgd");
      tl.w16[t] = nullptr;
      tl.w16_half[t] = false;
      if (!w16s.empty() && w16s[i].has_value()) {
        const at::Tensor& w16 = *w16s[i];
        TORCH_CHECK(w16.is_cuda() &&
                    (w16.scalar_type() == at::kBFloat16 ||
                     w16.scalar_type() == at::kHalf) &&
                    w16.sizes() == p.sizes() && w16.strides() == p.strides(),
                    "multi_tensor_sgd: w16 must be bf16 or fp16 in the "
                    "param's layout");
        tl.w16[t] = w16.data_ptr();
        tl.w16_half[t] = w16.scalar_type() == at::kHalf;
      }
    }
    auto kernel = ema ? (scaled ? multi_tensor_sgd_kernel<true, true>
                                : multi_tensor_sgd_kernel<false, true>)
                      : (scaled ? multi_tensor_sgd_kernel<true, false>
                                : multi_tensor_sgd_kernel<false, false>);
    hipLaunchKernelGGL(kernel,
                       dim3(b.nblocks), dim3(256), 0, stream, tl, (float)lr,
                       (float)momentum, (float)weight_decay, has_momentum,
                       gscale, scaled ? ratio + first : nullptr, dec.d,
                       dec.omd);
  }
}

void multi_tensor_sgd(std::vector<at::Tensor> params,
                      std::vector<at::Tensor> grads,
                      std::vector<at::Tensor> bufs,
                      double lr, double momentum, double weight_decay,
                      std::vector<c10::optional<at::Tensor>> w16s,
                      OptTensors emas, double ema_decay) {
  multi_tensor_sgd_impl(params, grads, bufs, lr, momentum, weight_decay, w16s,
                        nullptr, nullptr, emas, ema_decay);
}

// The two device coefficients of the scaled kernels: gscale [1], ratio [n].
static void check_coeffs(const at::Tensor& gscale, const at::Tensor& ratio,
                         size_t n, const at::Tensor& like) {
  TORCH_CHECK(gscale.is_cuda() && gscale.scalar_type() == at::kFloat &&
              gscale.numel() == 1 && gscale.device() == like.device(),
              "gscale must be one float32 on the params' device");
  TORCH_CHECK(ratio.is_cuda() && ratio.scalar_type() == at::kFloat &&
              ratio.is_contiguous() && (size_t)ratio.numel() == n &&
              ratio.device() == like.device(),
              "ratio must be a contiguous float32 [n], one per param");
}

void multi_tensor_sgd_scaled(std::vector<at::Tensor> params,
                             std::vector<at::Tensor> grads,
                             std::vector<at::Tensor> bufs,
                             double lr, double momentum, double weight_decay,
                             at::Tensor gscale, at::Tensor ratio,
                             std::vector<c10::optional<at::Tensor>> w16s,
                             OptTensors emas, double ema_decay) {
  if (params.empty()) return;
  check_coeffs(gscale, ratio, params.size(), params[0]);
  multi_tensor_sgd_impl(params, grads, bufs, lr, momentum, weight_decay, w16s,
                        gscale.data_ptr<float>(), ratio.data_ptr<float>(),
                        emas, ema_decay);
}

static void multi_tensor_sgd_o2_impl(std::vector<at::Tensor>& params,
                                     std::vector<at::Tensor>& grads,
                                     std::vector<at::Tensor>& masters,
                                     std::vector<at::Tensor>& bufs,
                                     double lr, double momentum,
                                     double weight_decay,
                                     const float* gscale, const float* ratio,
                                     const OptTensors& emas,
                                     double ema_decay) {
  const bool has_momentum = !bufs.empty();
  const bool scaled = gscale != nullptr;
  const bool ema = !emas.empty();
  const EmaDecay dec(ema_decay);
  TORCH_CHECK(params.size() == grads.size() &&
              params.size() == masters.size());
  TORCH_CHECK(!ema || emas.size() == params.size(),
              "multi_tensor_sgd_o2: one ema entry (or None) per param");
  TORCH_CHECK(!has_momentum || bufs.size() == params.size(),
              "multi_tensor_sgd_o2: one momentum buffer per param");
  auto stream = cur_stream();
  for (size_t i = 0; i < params.size();) {
    MTBatch<MTMixedList> b;
    MTMixedList& tl = b.tl;
    const size_t first = i;
    for (; !b.full() && i < params.size(); ++i) {
      auto& p = params[i];
      TORCH_CHECK(p.is_cuda() && p.is_non_overlapping_and_dense() &&
                  p.scalar_type() == at::ScalarType::BFloat16,
                  "multi_tensor_sgd_o2 expects dense bf16 params");
      TORCH_CHECK(grads[i].strides() == p.strides() &&
                  grads[i].scalar_type() == at::ScalarType::BFloat16,
                  "multi_tensor_sgd_o2: grad layout/dtype mismatch");
      TORCH_CHECK(masters[i].strides() == p.strides() &&
                  masters[i].scalar_type() == at::kFloat,
                  "multi_tensor_sgd_o2: master layout/dtype mismatch");
      const int t = b.push(p.numel());
      tl.p[t] = reinterpret_cast<__bf16*>(p.data_ptr());
      tl.g[t] = reinterpret_cast<const __bf16*>(grads[i].data_ptr());
      tl.w[t] = masters[i].data_ptr<float>();
      tl.m[t] = has_momentum ? bufs[i].data_ptr<float>() : nullptr;
      tl.ema[t] = ema_ptr(emas, i, masters[i], "multi_tensor_sgd_o2");
    }
    auto kernel = ema ? (scaled ? multi_tensor_sgd_o2_kernel<true, true>
                                : multi_tensor_sgd_o2_kernel<false, true>)
                      : (scaled ? multi_tensor_sgd_o2_kernel<true, false>
                                : multi_tensor_sgd_o2_kernel<false, false>);
    hipLaunchKernelGGL(kernel,
                       dim3(b.nblocks), dim3(256), 0, stream, tl, (float)lr,
                       (float)momentum, (float)weight_decay, has_momentum,
                       gscale, scaled ? ratio + first : nullptr, dec.d,
                       dec.omd);
  }
}

void multi_tensor_sgd_o2(std::vector<at::Tensor> params,
                         std::vector<at::Tensor> grads,
                         std::vector<at::Tensor> masters,
                         std::vector<at::Tensor> bufs,
                         double lr, double momentum, double weight_decay,
                         OptTensors emas, double ema_decay) {
  multi_tensor_sgd_o2_impl(params, grads, masters, bufs, lr, momentum,
                           weight_decay, nullptr, nullptr, emas, ema_decay);
}

void multi_tensor_sgd_o2_scaled(std::vector<at::Tensor> params,
                                std::vector<at::Tensor> grads,
                                std::vector<at::Tensor> masters,
                                std::vector<at::Tensor> bufs,
                                double lr, double momentum,
                                double weight_decay,
                                at::Tensor gscale, at::Tensor ratio,
                                OptTensors emas, double ema_decay) {
  if (params.empty()) return;
  check_coeffs(gscale, ratio, params.size(), params[0]);
  multi_tensor_sgd_o2_impl(params, grads, masters, bufs, lr, momentum,
                           weight_decay, gscale.data_ptr<float>(),
                           ratio.data_ptr<float>(), emas, ema_decay);
}

// emas[i] <- decay*emas[i] + (1 - decay)*srcs[i]; no allocation, no sync.
void multi_tensor_ema(std::vector<at::Tensor> srcs,
                      std::vector<at::Tensor> emas, double decay) {
  TORCH_CHECK(srcs.size() == emas.size(), "multi_tensor_ema: one ema per src");
  const EmaDecay dec(decay);
  auto stream = cur_stream();
  for (size_t i = 0; i < srcs.size();) {
    MTBatch<MTEmaList> b;
    for (; !b.full() && i < srcs.size(); ++i) {
      auto& s = srcs[i];
      auto& e = emas[i];
      TORCH_CHECK(s.is_cuda() && s.is_non_overlapping_and_dense() &&
                  s.scalar_type() == at::kFloat,
                  "multi_tensor_ema expects dense fp32 sources");
      TORCH_CHECK(e.is_cuda() && e.device() == s.device() &&
                  e.scalar_type() == at::kFloat && e.sizes() == s.sizes() &&
                  e.strides() == s.strides(),
                  "multi_tensor_ema: ema must be float32 in the source's "
                  "layout");
      const int t = b.push(s.numel());
      b.tl.src[t] = s.data_ptr<float>();
      b.tl.ema[t] = e.data_ptr<float>();
    }
    hipLaunchKernelGGL(multi_tensor_ema_kernel, dim3(b.nblocks), dim3(256), 0,
                       stream, b.tl, dec.d, dec.omd);
  }
}

// sq[0][i] <- sum w_i^2, sq[1][i] <- sum g_i^2 for every tensor, through
// `partials` ([2][>= total chunks]). Both buffers belong to the caller and
// nothing is allocated here. A launch holds gradients of one dtype, so the
// list is cut where the dtype changes as well as at MT_MAX_TENSORS.
void multi_tensor_sqnorm(std::vector<at::Tensor> ws,
                         std::vector<at::Tensor> gs,
                         at::Tensor partials, at::Tensor sq) {
  TORCH_CHECK(ws.size() == gs.size(), "multi_tensor_sqnorm: one g per w");
  if (ws.empty()) return;
  const int n = (int)ws.size();
  long total_chunks = 0;
  for (auto& w : ws) total_chunks += mt_chunks(w.numel());
  auto dev_f32 = [&](const at::Tensor& x) {
    return x.is_cuda() && x.scalar_type() == at::kFloat &&
           x.is_contiguous() && x.device() == ws[0].device();
  };
  TORCH_CHECK(dev_f32(partials) && partials.dim() == 2 &&
              partials.size(0) == 2 && partials.size(1) >= total_chunks,
              "multi_tensor_sqnorm: partials must be float32 [2][>= ",
              total_chunks, "]");
  TORCH_CHECK(dev_f32(sq) && sq.dim() == 2 && sq.size(0) == 2 &&
              sq.size(1) == n,
              "multi_tensor_sqnorm: sq must be float32 [2][", n, "]");
  const int pstride = (int)partials.size(1);
  auto stream = cur_stream();
  int chunk_base = 0;
  for (size_t i = 0; i < ws.size();) {
    MTBatch<MTNormList> b;
    MTNormList& tl = b.tl;
    const auto gdtype = gs[i].scalar_type();
    const int tensor_base = (int)i;
    for (; !b.full() && i < ws.size() && gs[i].scalar_type() == gdtype;
         ++i) {
      auto& w = ws[i];
      auto& g = gs[i];
      TORCH_CHECK(w.is_cuda() && w.is_non_overlapping_and_dense() &&
                  w.scalar_type() == at::kFloat &&
                  w.device() == ws[0].device(),
                  "multi_tensor_sqnorm expects dense fp32 weights");
      TORCH_CHECK(g.is_cuda() && g.is_non_overlapping_and_dense() &&
                  g.numel() == w.numel() && g.device() == w.device() &&
                  (gdtype == at::kFloat || gdtype == at::kBFloat16),
                  "multi_tensor_sqnorm expects dense fp32 or bf16 grads of "
                  "the weights' sizes");
      const int t = b.push(w.numel());
      tl.w[t] = w.data_ptr<float>();
      tl.g[t] = g.data_ptr();
    }
    if (b.nblocks > 0) {
      hipLaunchKernelGGL(gdtype == at::kFloat
                             ? multi_tensor_sqnorm_kernel<float>
                             : multi_tensor_sqnorm_kernel<__bf16>,
                         dim3(b.nblocks), dim3(256), 0, stream, tl,
                         partials.data_ptr<float>(), chunk_base, pstride);
    }
    hipLaunchKernelGGL(multi_tensor_sqnorm_fold_kernel, dim3(tl.ntensors),
                       dim3(256), 0, stream, tl, partials.data_ptr<float>(),
                       sq.data_ptr<float>(), chunk_base, pstride, tensor_base,
                       n);
    chunk_base += b.nblocks;
  }
}

// sq ([2][n], multi_tensor_sqnorm) -> gscale[0] = clip coefficient, gnorm =
// pre-clip global gradient norm, ratio[lo:hi] = LARS trust ratios.
void sgd_coeffs(at::Tensor sq, at::Tensor excluded, at::Tensor gscale,
                at::Tensor ratio, at::Tensor gnorm, double max_norm, bool lars,
                double eta, double weight_decay, int64_t lo, int64_t hi) {
  TORCH_CHECK(sq.is_cuda() && sq.scalar_type() == at::kFloat &&
              sq.is_contiguous() && sq.dim() == 2 && sq.size(0) == 2,
              "sgd_coeffs: sq must be a contiguous float32 [2][n]");
  const int64_t n = sq.size(1);
  if (hi < 0) hi = n;
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= n, "sgd_coeffs: bad range");
  TORCH_CHECK(excluded.is_cuda() && excluded.scalar_type() == at::kByte &&
              excluded.is_contiguous() && excluded.numel() == n &&
              excluded.device() == sq.device(),
              "sgd_coeffs: excluded must be uint8 [n]");
  check_coeffs(gscale, ratio, (size_t)n, sq);
  TORCH_CHECK(gnorm.is_cuda() && gnorm.scalar_type() == at::kFloat &&
              gnorm.numel() == 1 && gnorm.device() == sq.device(),
              "sgd_coeffs: gnorm must be one float32");
  hipLaunchKernelGGL(sgd_coeffs_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     sq.data_ptr<float>(), excluded.data_ptr<unsigned char>(),
                     gscale.data_ptr<float>(), ratio.data_ptr<float>(),
                     gnorm.data_ptr<float>(), (int)n, (int)lo, (int)hi,
                     (float)max_norm, lars, (float)eta, (float)weight_decay);
}

at::Tensor multi_tensor_unscale(std::vector<at::Tensor> grads, double inv_scale) {
  TORCH_CHECK(!grads.empty());
  auto found = at::zeros({1}, grads[0].options().dtype(at::kInt));
  auto stream = cur_stream();
  for (size_t i = 0; i < grads.size();) {
    MTBatch<MTGradList> b;
    for (; !b.full() && i < grads.size(); ++i) {
      TORCH_CHECK(grads[i].is_cuda() && grads[i].is_non_overlapping_and_dense() &&
                  grads[i].scalar_type() == at::kFloat,
                  "multi_tensor_unscale expects dense fp32 grads");
      b.tl.g[b.push(grads[i].numel())] = grads[i].data_ptr<float>();
    }
    hipLaunchKernelGGL(multi_tensor_unscale_kernel, dim3(b.nblocks), dim3(256),
                       0, stream, b.tl, (float)inv_scale,
                       found.data_ptr<int>());
  }
  return found;
}

at::Tensor gap_fwd(at::Tensor x) {
  CHECK_CUDA(x); check_dense(x, "x");
  const int N = x.size(0), C = x.size(1);
  const int S = x.numel() / ((long)N * C);
  auto y = at::empty({N, C, 1, 1},
                     is_clast(x)
                         ? x.options().memory_format(at::MemoryFormat::ChannelsLast)
                         : x.options());
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "gap_fwd", [&] {
    if (is_clast(x)) {
      hipLaunchKernelGGL(gap_fwd_nhwc_kernel<scalar_t>,
                         dim3((C + 255) / 256, N), dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(), C, S);
    } else {
      hipLaunchKernelGGL(gap_fwd_nchw_kernel<scalar_t>, dim3((long)N * C),
                         dim3(256), 0, cur_stream(),
                         x.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(), C, S);
    }
  });
  return y;
}

at::Tensor gap_bwd(at::Tensor dy, at::Tensor x_like) {
  CHECK_CUDA(dy);
  const int N = x_like.size(0), C = x_like.size(1);
  const int S = x_like.numel() / ((long)N * C);
  const long total = x_like.numel();
  auto fmt = is_clast(x_like) ? at::MemoryFormat::ChannelsLast
                              : at::MemoryFormat::Contiguous;
  auto dx = at::empty_like(x_like, x_like.options().memory_format(fmt));
  auto dyc = dy.reshape({N, C}).contiguous();
  const int blocks = (int)std::min((total + 255) / 256, (long)4096);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      dy.scalar_type(), "gap_bwd", [&] {
    auto launch = [&](auto cl_c) {
      hipLaunchKernelGGL((gap_bwd_kernel<scalar_t, decltype(cl_c)::value>),
                         dim3(blocks), dim3(256), 0, cur_stream(),
                         dyc.data_ptr<scalar_t>(), dx.data_ptr<scalar_t>(),
                         total, C, S);
    };
    is_clast(x_like) ? launch(std::true_type{}) : launch(std::false_type{});
  });
  return dx;
}

std::vector<at::Tensor> maxpool_fwd(at::Tensor x, long k, long stride,
                                    long pad) {
  CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4 &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "maxpool_fwd expects NHWC (channels_last)");
  const int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C % 8 == 0, "maxpool_fwd needs C % 8 == 0");
  const int P = (H + 2 * (int)pad - (int)k) / (int)stride + 1;
  const int Q = (W + 2 * (int)pad - (int)k) / (int)stride + 1;
  auto y = at::empty({Nb, C, P, Q},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto idx = at::empty({(long)Nb * P * Q * C}, x.options().dtype(at::kByte));
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      x.scalar_type(), "maxpool_fwd", [&] {
    const long nvec = (long)Nb * P * Q * C / (16 / sizeof(scalar_t));
    const int blocks = (int)std::min((nvec + 255) / 256, (long)4096);
    hipLaunchKernelGGL(maxpool_fwd_nhwc_kernel<scalar_t>,
                       dim3(std::max(blocks, 1)), dim3(256), 0, cur_stream(),
                       x.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(),
                       idx.data_ptr<unsigned char>(), Nb, H, W, C, P, Q,
                       (int)k, (int)stride, (int)pad);
  });
  return {y, idx};
}

at::Tensor maxpool_bwd(at::Tensor dy, at::Tensor idx, long H, long W,
                       long k, long stride, long pad) {
  CHECK_CUDA(dy);
  TORCH_CHECK(dy.dim() == 4 &&
              dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "maxpool_bwd expects NHWC dy");
  const int Nb = dy.size(0), C = dy.size(1), P = dy.size(2), Q = dy.size(3);
  auto dx = at::empty({Nb, C, (long)H, (long)W},
                      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      dy.scalar_type(), "maxpool_bwd", [&] {
    const long nvec = (long)Nb * H * W * C / (16 / sizeof(scalar_t));
    const int blocks = (int)std::min((nvec + 255) / 256, (long)4096);
    hipLaunchKernelGGL(maxpool_bwd_nhwc_kernel<scalar_t>,
                       dim3(std::max(blocks, 1)), dim3(256), 0, cur_stream(),
                       dy.data_ptr<scalar_t>(), idx.data_ptr<unsigned char>(),
                       dx.data_ptr<scalar_t>(), Nb, (int)H, (int)W, C, P, Q,
                       (int)k, (int)stride, (int)pad);
  });
  return dx;
}

at::Tensor class_rank(at::Tensor logits, at::Tensor target) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  CHECK_CUDA(target); CHECK_CONTIG(target);
  TORCH_CHECK(target.scalar_type() == at::kLong, "target must be int64");
  TORCH_CHECK(target.numel() == logits.size(0),
              "target must have one entry per logits row");
  const int N = logits.size(0), C = logits.size(1);
  auto rank = at::empty({N}, logits.options().dtype(at::kInt));
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::Half, at::ScalarType::BFloat16,
      logits.scalar_type(), "class_rank", [&] {
    hipLaunchKernelGGL(class_rank_kernel<scalar_t>, dim3(N),
                       dim3(C <= 128 ? 64 : 256), 0, cur_stream(),
                       logits.data_ptr<scalar_t>(), target.data_ptr<long>(),
                       rank.data_ptr<int>(), N, C);
  });
  return rank;
}

// csrc/conv_igemm.hip — implicit-GEMM MFMA convolution (NHWC bf16 or fp16)
at::Tensor conv_build_wT(at::Tensor w);
at::Tensor conv_fwd_igemm(at::Tensor x, at::Tensor w, long stride, long pad,
                          long tile, long splits);
at::Tensor conv_fwd_bn_igemm(at::Tensor x, at::Tensor w,
                             at::Tensor scale_shift,
                             c10::optional<at::Tensor> residual, bool relu,
                             long stride, long pad, long tile, long splits);
at::Tensor conv_dgrad_igemm(at::Tensor dy, at::Tensor wT, long H, long W,
                            long stride, long pad, long tile, long splits);
at::Tensor conv_wgrad_igemm(at::Tensor dy, at::Tensor x, long R, long S,
                            long stride, long pad, long splits, long wtile,
                            bool out_fp32);
void multi_tensor_build_wT(std::vector<at::Tensor> w16s,
                           std::vector<at::Tensor> wTs);
void conv_prep_weight(at::Tensor w32, at::Tensor w16, at::Tensor wT);

// csrc/data_aug.hip — device-resident input pipeline (crop/flip/normalize)
std::tuple<at::Tensor, at::Tensor> batch_augment(
    at::Tensor images_u8, at::Tensor labels_i64, at::Tensor idx_i32,
    c10::optional<at::Tensor> aug_i32, at::Tensor lut_f32, long pad,
    bool channels_last, at::ScalarType out_dtype);
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> batch_augment_cutmix(
    at::Tensor images_u8, at::Tensor labels_i64, at::Tensor idx_i32,
    c10::optional<at::Tensor> aug_i32, at::Tensor mix_i32, at::Tensor lam_f32,
    at::Tensor lut_f32, long pad, bool channels_last,
    at::ScalarType out_dtype);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("conv_build_wT", &conv_build_wT,
        "build rotated/transposed filter for dgrad (one launch)");
  m.def("conv_fwd_igemm", &conv_fwd_igemm,
        "implicit-GEMM conv forward (NHWC bf16|fp16, MFMA); "
        "tile 0=auto|64|128|228 (128x128); splits > 1 with tile 228: split-K "
        "slices + one reduce",
        py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"),
        py::arg("tile") = 0, py::arg("splits") = 1);
  m.def("conv_fwd_bn_igemm", &conv_fwd_bn_igemm,
        "conv_fwd_igemm with eval-mode BatchNorm (+residual)(+relu) applied "
        "to the fp32 accumulator: scale_shift is fp32 [4][K], rows 2, 3 = "
        "scale, shift; tile and splits as in conv_fwd_igemm",
        py::arg("x"), py::arg("w"), py::arg("scale_shift"),
        py::arg("residual") = py::none(), py::arg("relu") = false,
        py::arg("stride") = 1, py::arg("pad") = 0, py::arg("tile") = 0,
        py::arg("splits") = 1);
  m.def("conv_dgrad_igemm", &conv_dgrad_igemm,
        "implicit-GEMM conv input-grad (NHWC bf16|fp16, MFMA); "
        "tile 0=auto|64|128|228 (128x128); splits > 1 with tile 228: split-K "
        "slices + one reduce (not on the stride-2 parity path)",
        py::arg("dy"), py::arg("wT"), py::arg("H"), py::arg("W"),
        py::arg("stride"), py::arg("pad"), py::arg("tile") = 0,
        py::arg("splits") = 1);
  m.def("conv_wgrad_igemm", &conv_wgrad_igemm,
        "implicit-GEMM conv weight-grad -> channels_last (K,C,R,S) in the "
        "input dtype; "
        "two-stage split-K, no atomics; splits 0=auto; wtile 0=auto, "
        "1=64x128, 2=128x128, 3=256x64; out_fp32: the same 16-bit-rounded "
        "values as an fp32 tensor",
        py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"),
        py::arg("stride"), py::arg("pad"), py::arg("splits") = 0,
        py::arg("wtile") = 0, py::arg("out_fp32") = false);
  m.def("multi_tensor_build_wT", &multi_tensor_build_wT,
        "wT[i] <- rotated/transposed w16[i] for every filter, one launch");
  m.def("conv_prep_weight", &conv_prep_weight,
        "w16 <- w32 rounded to w16.dtype (bf16|fp16) and wT <- "
        "rotated/transposed w16, one launch");
  m.def("bn_stats", &bn_stats, "per-channel sum/sqsum (NCHW)");
  m.def("bn_stats_packed", &bn_stats_packed,
        "per-channel {sum,sqsum} packed [2C], no-atomic NHWC v2");
  m.def("bn_finalize", &bn_finalize,
        "packed stats + count -> mean/invstd (+running update), one launch");
  m.def("bn_bwd_reduce_packed", &bn_bwd_reduce_packed,
        "BN backward reductions packed [2C] w/ relu mask");
  m.def("bn_fwd", &bn_fwd, "fused BN(+add)(+relu) forward");
  m.def("bn_bwd_reduce", &bn_bwd_reduce, "BN backward reductions w/ relu mask");
  m.def("bn_bwd", &bn_bwd, "BN backward apply");
  m.def("bn_v2_ok", &bn_v2_ok, "x takes the NHWC v2 partial/tail path");
  m.def("bn_stats_partial", &bn_stats_partial,
        "NHWC v2 {sum,sqsum} partial [split][2C], unreduced");
  m.def("bn_fwd_tail", &bn_fwd_tail,
        "partial -> {stats [4][C], mean, invstd} + running stats, one launch");
  m.def("bn_fwd_apply", &bn_fwd_apply,
        "fused BN(+add)(+relu) forward from bn_fwd_tail's stats");
  m.def("bn_bwd_reduce_partial", &bn_bwd_reduce_partial,
        "NHWC v2 {sum_dy,sum_dy_xhat} partial [split][2C], unreduced");
  m.def("bn_bwd_tail", &bn_bwd_tail,
        "partial -> {dbeta, dgamma, coeffs [3][C]}, one launch");
  m.def("bn_bwd_tail_dup", &bn_bwd_tail_dup,
        "partial -> {dbeta, dgamma, packed [2C]} for the SyncBN all_reduce");
  m.def("bn_bwd_apply", &bn_bwd_apply,
        "BN backward apply from bn_bwd_tail's coeffs");
  m.def("xent_fwd", &xent_fwd, "fused softmax cross-entropy forward");
  m.def("xent_bwd", &xent_bwd, "fused softmax cross-entropy backward");
  m.def("xent_mix_fwd", &xent_mix_fwd,
        "two-label smoothed cross-entropy forward: lam*CE(a) + (1-lam)*CE(b) "
        "with label smoothing eps -> (loss, lse)",
        py::arg("logits"), py::arg("target_a"), py::arg("target_b"),
        py::arg("lam"), py::arg("eps"));
  m.def("xent_mix_bwd", &xent_mix_bwd,
        "two-label smoothed cross-entropy backward",
        py::arg("logits"), py::arg("target_a"), py::arg("target_b"),
        py::arg("lam"), py::arg("lse"), py::arg("dloss"), py::arg("eps"));
  m.def("multi_tensor_sgd", &multi_tensor_sgd,
        "fused multi-tensor SGD step; w16s: per-param bf16|fp16 shadow (or "
        "None) "
        "that receives the rounded new weight",
        py::arg("params"), py::arg("grads"), py::arg("bufs"), py::arg("lr"),
        py::arg("momentum"), py::arg("weight_decay"),
        py::arg("w16s") = OptTensors(), py::arg("emas") = OptTensors(),
        py::arg("ema_decay") = 0.0);
  m.def("multi_tensor_sgd_o2", &multi_tensor_sgd_o2,
        "fused SGD with bf16 params/grads + fp32 master (apex O2); emas: "
        "per-param fp32 average of the master (or None)",
        py::arg("params"), py::arg("grads"), py::arg("masters"),
        py::arg("bufs"), py::arg("lr"), py::arg("momentum"),
        py::arg("weight_decay"), py::arg("emas") = OptTensors(),
        py::arg("ema_decay") = 0.0);
  m.def("multi_tensor_ema", &multi_tensor_ema,
        "emas[i] <- decay*emas[i] + (1 - decay)*srcs[i], fp32, in one launch "
        "per 32 tensors; srcs are not modified",
        py::arg("srcs"), py::arg("emas"), py::arg("decay"));
  m.def("multi_tensor_sqnorm", &multi_tensor_sqnorm,
        "per-tensor sums of squares of w (fp32) and g (fp32|bf16) -> sq "
        "[2][n] through partials [2][>= chunks]; fixed order, no atomics",
        py::arg("ws"), py::arg("gs"), py::arg("partials"), py::arg("sq"));
  m.def("sgd_coeffs", &sgd_coeffs,
        "sq -> gscale[0] = min(1, max_norm/(|g| + 1e-6)) (1 when max_norm <= "
        "0), gnorm = |g|, ratio[lo:hi] = LARS trust ratios (1 when lars is "
        "off, excluded, or a norm is 0)",
        py::arg("sq"), py::arg("excluded"), py::arg("gscale"),
        py::arg("ratio"), py::arg("gnorm"), py::arg("max_norm"),
        py::arg("lars"), py::arg("eta"), py::arg("weight_decay"),
        py::arg("lo") = 0, py::arg("hi") = -1);
  m.def("multi_tensor_sgd_scaled", &multi_tensor_sgd_scaled,
        "multi_tensor_sgd with d = ratio[t]*(gscale[0]*g + wd*p) read from "
        "device memory; g is not modified",
        py::arg("params"), py::arg("grads"), py::arg("bufs"), py::arg("lr"),
        py::arg("momentum"), py::arg("weight_decay"), py::arg("gscale"),
        py::arg("ratio"), py::arg("w16s") = OptTensors(),
        py::arg("emas") = OptTensors(), py::arg("ema_decay") = 0.0);
  m.def("multi_tensor_sgd_o2_scaled", &multi_tensor_sgd_o2_scaled,
        "multi_tensor_sgd_o2 with d = ratio[t]*(gscale[0]*g + wd*master)",
        py::arg("params"), py::arg("grads"), py::arg("masters"),
        py::arg("bufs"), py::arg("lr"), py::arg("momentum"),
        py::arg("weight_decay"), py::arg("gscale"), py::arg("ratio"),
        py::arg("emas") = OptTensors(), py::arg("ema_decay") = 0.0);
  m.def("multi_tensor_unscale", &multi_tensor_unscale,
        "multi-tensor grad unscale + inf/nan check");
  // ops/sgd.py keeps its own values for the CPU fallback; a test compares them
  m.attr("MT_CHUNK") = MT_CHUNK;
  m.attr("MT_MAX_TENSORS") = MT_MAX_TENSORS;
  m.attr("LARS_EPS") = LARS_EPS;
  m.attr("CLIP_EPS") = CLIP_EPS;
  m.def("gap_fwd", &gap_fwd, "global average pool forward (NCHW/NHWC)");
  m.def("gap_bwd", &gap_bwd, "global average pool backward");
  m.def("maxpool_fwd", &maxpool_fwd,
        "NHWC max pool forward -> (y, argmax idx)");
  m.def("maxpool_bwd", &maxpool_bwd, "NHWC max pool backward (gather)");
  m.def("class_rank", &class_rank, "per-row rank of target class (for top-k)");
  m.def("batch_augment", &batch_augment,
        "uint8 NHWC dataset + batch indices -> (images, labels): zero-padded "
        "crop, flip, table normalize and cast in one launch; aug None = eval",
        py::arg("images_u8"), py::arg("labels_i64"), py::arg("idx_i32"),
        py::arg("aug_i32"), py::arg("lut_f32"), py::arg("pad"),
        py::arg("channels_last"), py::arg("out_dtype"));
  m.def("batch_augment_cutmix", &batch_augment_cutmix,
        "batch_augment with a CutMix box per sample: mix[i] = (partner dataset "
        "index or -1, y0|y1<<16, x0|x1<<16), lam[i] -> (images, labels_a, "
        "labels_b, lam)",
        py::arg("images_u8"), py::arg("labels_i64"), py::arg("idx_i32"),
        py::arg("aug_i32"), py::arg("mix_i32"), py::arg("lam_f32"),
        py::arg("lut_f32"), py::arg("pad"), py::arg("channels_last"),
        py::arg("out_dtype"));
}
