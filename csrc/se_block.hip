// MI355X (gfx950/CDNA4) Squeeze-and-Excitation join (Hu et al. 2018):
//   out = relu(u * g[n, c] + identity),  g = sigmoid(W2 relu(W1 s + b1) + b2),
//   s[n, c] = mean_hw u
// u, identity, out: NHWC bf16 or fp16, C a multiple of 8. The whole gate path
// is fp32: s, h, g, their gradients and the four parameter gradients never
// pass through a 16-bit value, and W1 [Cr, C], b1, W2 [C, Cr], b2 are the fp32
// master parameters read as they are (no shadow, no cast).
//
// Forward, three launches; backward, four. Saved: u, out, s, h, g.
//
// se_reduce_kernel (se_squeeze, se_join_bwd_reduce). The work split of the
// depthwise kernels: a block of 256 threads owns a 64-channel chunk of NI
// images; tid & 7 is a lane's 8 consecutive channels (every access of an
// activation is 16 bytes), tid >> 3 one of 32 pixel slots, 32 / NI per image,
// striding over HW. The slots are folded through LDS in slot order: no
// atomics, a fixed sum order. NI by HW: 1 pixel 32 images, up to 4 pixels 8,
// up to 16 pixels 2, else 1, so the late small stages run full blocks.
// The backward form sums (out > 0) * dout * u instead of u.
//
// se_excite_fwd_kernel / se_excite_bwd_kernel. A block owns 16 images, the M
// tile of v_mfma_f32_16x16x4_f32; its four waves split the 16-wide column
// tiles. A lane (i = lane & 15, q = lane >> 4) feeds four MFMAs from one group
// of 16 k: its k are 4q .. 4q+3 of the group, for A and for B alike, so the A
// operand is one 16-byte LDS read (and FC1's W1 row one 16-byte global read).
//   fwd  FC1: K = C, s staged through LDS in chunks of 256 k (never whole),
//             bias + ReLU, h to LDS [16][Cr16 + 4] and to global;
//        FC2: K = Cr from LDS, bias + sigmoid, g to global.
//   bwd  dz2 = dg * g(1-g) is formed while staging the A chunk (and stored);
//        dz1 = (dz2 W2) * (h > 0), K = C, to LDS and global;
//        ds  = dz1 W1, K = Cr from LDS.
// Only N / 16 blocks run, so what hides the latency of the weight stream is
// the loads a wave has in flight: the B operands of 8 groups of two column
// tiles (first GEMM), of 4 groups of four tiles (second), are issued before
// their MFMAs, which also gives every MFMA chain an independent neighbour.
// The weights stream from global memory (L2-resident across blocks). Ragged
// N, Cr and C/16 are predicated loads of zeros and predicated stores.
//
// se_excite_wgrad_kernel. One wave per 16 x 16 tile of dW2 = dz2^T h or dW1 =
// dz1^T s, contracting over the whole batch in image order with the same MFMA
// (K = N, the ragged last step predicated). The tiles of the first column
// tile also run a second MFMA against ones: its column 0 is db. No atomics,
// no slab, no reduce pass; bit-reproducible.
//
// se_scale_add_relu_kernel / se_join_bwd_apply_kernel. Elementwise, one
// 16-byte lane per thread, fp32 math, one rounding, vector stores:
//   out = relu(u * g + identity)
//   d_identity = m * dout,  du = m * dout * g + ds[n, c] / HW,  m = out > 0
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <tuple>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int CHUNK = 64;   // channels per reduce block
constexpr int SLOTS = 32;   // pixel slots per reduce block
constexpr int MT = 16;      // images per excite block: one MFMA M tile
constexpr int KC = 256;     // k per staged chunk of the A operand
constexpr int LDA = KC + 4; // its padded row, in floats
constexpr int GU = 8;       // groups of 16 k whose B loads are in flight at once
constexpr int MAX_CR = 512; // h [16][Cr16 + 4] and the chunk stay under 64 KB

template <typename T>
__device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8]) {
  typedef __attribute__((ext_vector_type(8))) T x8;
  const x8 e = __builtin_bit_cast(x8, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (float)e[i];
}

template <typename T>
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  typedef __attribute__((ext_vector_type(8))) T x8;
  x8 e;
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = (T)f[i];
  return __builtin_bit_cast(u32x4, e);
}

// ---------------------------------------------------------------------------
// [N, C] fp32 reductions over HW
// ---------------------------------------------------------------------------
// grid (ceil(N / NI), ceil(C / 64)). dst[n, c] = scale * sum_hw (BWD ? (out >
// 0) * dout * u : u).
template <typename T, int NI, bool BWD>
__global__ __launch_bounds__(256)
void se_reduce_kernel(const T* __restrict__ u, const T* __restrict__ out,
                      const T* __restrict__ dout, float* __restrict__ dst,
                      int N, int C, int HW, float scale) {
  constexpr int SPI = SLOTS / NI;   // slots per image
  __shared__ float f[SLOTS * CHUNK];
  const int cl = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int n = blockIdx.x * NI + slot / SPI;
  const int ch = blockIdx.y * CHUNK + cl * 8;

  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (n < N && ch < C) {
    const size_t base = (size_t)n * HW * C + ch;
#pragma unroll 4
    for (int p = slot % SPI; p < HW; p += SPI) {
      const size_t v = (base + (size_t)p * C) >> 3;
      float a[8];
      unpack8<T>(reinterpret_cast<const u32x4*>(u)[v], a);
      if constexpr (BWD) {
        float o[8], d[8];
        unpack8<T>(reinterpret_cast<const u32x4*>(out)[v], o);
        unpack8<T>(reinterpret_cast<const u32x4*>(dout)[v], d);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          acc[i] += o[i] > 0.f ? d[i] * a[i] : 0.f;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += a[i];
      }
    }
  }
  f32x4* fd = reinterpret_cast<f32x4*>(f + slot * CHUNK + cl * 8);
  fd[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  fd[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  __syncthreads();
  // fold an image's slots in slot order
  for (int e = threadIdx.x; e < NI * CHUNK; e += 256) {
    const int img = e >> 6, cc = e & 63;
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < SPI; ++s) sum += f[(img * SPI + s) * CHUNK + cc];
    const int nn = blockIdx.x * NI + img, c = blockIdx.y * CHUNK + cc;
    if (nn < N && c < C) dst[(size_t)nn * C + c] = sum * scale;
  }
}

// ---------------------------------------------------------------------------
// elementwise joins; one 16-byte lane per thread, nvec < 2^31
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
  const f32x4 a = reinterpret_cast<const f32x4*>(p)[0];
  const f32x4 b = reinterpret_cast<const f32x4*>(p)[1];
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
  f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

template <typename T>
__global__ __launch_bounds__(256)
void se_scale_add_relu_kernel(const T* __restrict__ u, const T* __restrict__ idn,
                              const float* __restrict__ g, T* __restrict__ out,
                              unsigned nvec, unsigned C8, unsigned img_vecs) {
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= nvec) return;
  const unsigned n = v / img_vecs, c8 = v % C8;
  float a[8], r[8], gg[8];
  unpack8<T>(reinterpret_cast<const u32x4*>(u)[v], a);
  unpack8<T>(reinterpret_cast<const u32x4*>(idn)[v], r);
  load8(g + ((size_t)n * C8 + c8) * 8, gg);
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = fmaxf(fmaf(a[i], gg[i], r[i]), 0.f);
  reinterpret_cast<u32x4*>(out)[v] = pack8<T>(a);
}

template <typename T>
__global__ __launch_bounds__(256)
void se_join_bwd_apply_kernel(const T* __restrict__ dout,
                              const T* __restrict__ out,
                              const float* __restrict__ g,
                              const float* __restrict__ ds, T* __restrict__ du,
                              T* __restrict__ didn, unsigned nvec, unsigned C8,
                              unsigned img_vecs, float inv_hw) {
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= nvec) return;
  const unsigned n = v / img_vecs, c8 = v % C8;
  float d[8], o[8], gg[8], s[8];
  unpack8<T>(reinterpret_cast<const u32x4*>(dout)[v], d);
  unpack8<T>(reinterpret_cast<const u32x4*>(out)[v], o);
  load8(g + ((size_t)n * C8 + c8) * 8, gg);
  load8(ds + ((size_t)n * C8 + c8) * 8, s);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    d[i] = o[i] > 0.f ? d[i] : 0.f;
    o[i] = fmaf(d[i], gg[i], s[i] * inv_hw);
  }
  reinterpret_cast<u32x4*>(didn)[v] = pack8<T>(d);
  reinterpret_cast<u32x4*>(du)[v] = pack8<T>(o);
}

// ---------------------------------------------------------------------------
// the two FC layers on v_mfma_f32_16x16x4_f32
// ---------------------------------------------------------------------------
// D[i][j] += sum_k A[i][k] B[k][j]: a lane holds A[lane & 15][lane >> 4],
// B[lane >> 4][lane & 15] and D[4 * (lane >> 4) + r][lane & 15], r = 0..3.
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One group of 16 k: the lane's a[t], b[t] are k = 4q + t of the group.
__device__ __forceinline__ f32x4 mfma_group(f32x4 a, f32x4 b, f32x4 c) {
  c = mfma4(a[0], b[0], c);
  c = mfma4(a[1], b[1], c);
  c = mfma4(a[2], b[2], c);
  return mfma4(a[3], b[3], c);
}

// a_lds [16][LDA] <- rows n0.. of the [N, C] operand, columns kc.. (zeros past
// N and C). GRAD: the operand is dz2 = dg * g(1-g), formed here and stored
// when `store`.
template <bool GRAD>
__device__ __forceinline__ void stage_a(float* a_lds, const float* src,
                                        const float* g, float* dz2, bool store,
                                        int n0, int kc, int N, int C) {
  for (int e = threadIdx.x; e < MT * KC / 4; e += 256) {
    const int i = e / (KC / 4), k4 = (e % (KC / 4)) * 4;
    const int n = n0 + i, k = kc + k4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < N && k < C) {
      const size_t at = (size_t)n * C + k;
      v = *reinterpret_cast<const f32x4*>(src + at);
      if constexpr (GRAD) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + at);
        v = v * gg * (1.f - gg);
        if (store) *reinterpret_cast<f32x4*>(dz2 + at) = v;
      }
    }
    *reinterpret_cast<f32x4*>(a_lds + i * LDA + k4) = v;
  }
}

// The second GEMM of both passes: D = hl [16][K = Cr16] . B with B[k][c] =
// W[k * sk + c * sc], k < Cr, over the column tiles of C; fin(value, c) is
// what is stored at dst[n, c].
template <typename Fin>
__device__ __forceinline__ void fc_from_lds(const float* hl, int ldh,
                                            const float* __restrict__ W,
                                            size_t sk, size_t sc,
                                            float* __restrict__ dst, int n0,
                                            int N, int C, int Cr, Fin fin) {
  // A wave takes TP column tiles at a time and issues the B loads of GU
  // groups of all of them before their MFMAs: few waves run, so the loads in
  // flight per wave are what hides the latency of global memory.
  constexpr int TP = 4, GU = 4;   // (this GEMM's own batch of groups)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, q = lane >> 4;
  const int Crp = (Cr + 15) & ~15;
  for (int ct0 = wave * TP; ct0 < (C + 15) / 16; ct0 += 4 * TP) {
    f32x4 acc[TP];
#pragma unroll
    for (int p = 0; p < TP; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Crp; k0 += 16 * GU) {
      f32x4 b[TP][GU];
#pragma unroll
      for (int p = 0; p < TP; ++p) {
        const int c = (ct0 + p) * 16 + li;   // a tile past C loads zeros
#pragma unroll
        for (int gi = 0; gi < GU; ++gi) {
          const int k = k0 + 16 * gi + 4 * q;
#pragma unroll
          for (int t = 0; t < 4; ++t)
            b[p][gi][t] = (c < C && k + t < Cr)
                ? W[(size_t)(k + t) * sk + (size_t)c * sc] : 0.f;
        }
      }
#pragma unroll
      for (int gi = 0; gi < GU; ++gi) {
        if (k0 + 16 * gi < Crp) {            // the same in all of a wave
          const f32x4 a = *reinterpret_cast<const f32x4*>(
              hl + li * ldh + k0 + 16 * gi + 4 * q);
#pragma unroll
          for (int p = 0; p < TP; ++p) acc[p] = mfma_group(a, b[p][gi], acc[p]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < TP; ++p) {
      const int c = (ct0 + p) * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * q + r;
        if (n < N && c < C) dst[(size_t)n * C + c] = fin(acc[p][r], c);
      }
    }
  }
}

// grid ceil(N / 16); dynamic LDS (16 * LDA + 16 * (Cr16 + 4)) floats.
__global__ __launch_bounds__(256)
void se_excite_fwd_kernel(const float* __restrict__ s,
                          const float* __restrict__ W1,
                          const float* __restrict__ b1,
                          const float* __restrict__ W2,
                          const float* __restrict__ b2, float* __restrict__ h,
                          float* __restrict__ g, int N, int C, int Cr) {
  extern __shared__ float smem[];
  float* a_lds = smem;
  float* hl = smem + MT * LDA;
  const int Crp = (Cr + 15) & ~15, ldh = Crp + 4, rtiles = Crp >> 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * MT;

  // FC1: eight column tiles of Cr per pass, two per wave
  for (int jt0 = 0; jt0 < rtiles; jt0 += 8) {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kc = 0; kc < C; kc += KC) {
      __syncthreads();   // the previous chunk's readers are done
      stage_a<false>(a_lds, s, nullptr, nullptr, false, n0, kc, N, C);
      __syncthreads();
      const int klen = min(KC, C - kc);
      // the B loads of GU groups of both tiles are issued before their MFMAs
      for (int k0 = 0; k0 < klen; k0 += 16 * GU) {
        f32x4 b[2][GU];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int j = (jt0 + 4 * t + wave) * 16 + li;   // past Cr: zeros
#pragma unroll
          for (int gi = 0; gi < GU; ++gi) {
            const int k = kc + k0 + 16 * gi + 4 * q;
            b[t][gi] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < Cr && k < C)             // C % 4 == 0: all four or none
              b[t][gi] =
                  *reinterpret_cast<const f32x4*>(W1 + (size_t)j * C + k);
          }
        }
#pragma unroll
        for (int gi = 0; gi < GU; ++gi) {    // k0 + 16 gi + 4q + 3 < KC
          const f32x4 a = *reinterpret_cast<const f32x4*>(
              a_lds + li * LDA + k0 + 16 * gi + 4 * q);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t] = mfma_group(a, b[t][gi], acc[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int jt = jt0 + 4 * t + wave;
      if (jt >= rtiles) continue;
      const int j = jt * 16 + li;
      const float bias = j < Cr ? b1[j] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * q + r, n = n0 + i;
        const float v = j < Cr ? fmaxf(acc[t][r] + bias, 0.f) : 0.f;
        hl[i * ldh + j] = v;
        if (n < N && j < Cr) h[(size_t)n * Cr + j] = v;
      }
    }
  }
  __syncthreads();
  // FC2: B[k][c] = W2[c * Cr + k]
  fc_from_lds(hl, ldh, W2, 1, (size_t)Cr, g, n0, N, C, Cr,
              [b2](float z, int c) { return 1.f / (1.f + expf(-(z + b2[c]))); });
}

// grid ceil(N / 16); the same LDS.
__global__ __launch_bounds__(256)
void se_excite_bwd_kernel(const float* __restrict__ dg,
                          const float* __restrict__ g,
                          const float* __restrict__ h,
                          const float* __restrict__ W1,
                          const float* __restrict__ W2, float* __restrict__ dz2,
                          float* __restrict__ dz1, float* __restrict__ ds,
                          int N, int C, int Cr) {
  extern __shared__ float smem[];
  float* a_lds = smem;
  float* hl = smem + MT * LDA;
  const int Crp = (Cr + 15) & ~15, ldh = Crp + 4, rtiles = Crp >> 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * MT;

  // dz1 = (dz2 W2) * (h > 0): K = C, B[k][j] = W2[k * Cr + j]
  for (int jt0 = 0; jt0 < rtiles; jt0 += 8) {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kc = 0; kc < C; kc += KC) {
      __syncthreads();
      stage_a<true>(a_lds, dg, g, dz2, jt0 == 0, n0, kc, N, C);
      __syncthreads();
      const int klen = min(KC, C - kc);
      for (int k0 = 0; k0 < klen; k0 += 16 * GU) {
        f32x4 b[2][GU];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int j = (jt0 + 4 * t + wave) * 16 + li;
#pragma unroll
          for (int gi = 0; gi < GU; ++gi) {
            const int k = kc + k0 + 16 * gi + 4 * q;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)   // k % 4 == 0 == C % 4
              b[t][gi][tt] = (j < Cr && k < C)
                                 ? W2[(size_t)(k + tt) * Cr + j] : 0.f;
          }
        }
#pragma unroll
        for (int gi = 0; gi < GU; ++gi) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(
              a_lds + li * LDA + k0 + 16 * gi + 4 * q);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t] = mfma_group(a, b[t][gi], acc[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int jt = jt0 + 4 * t + wave;
      if (jt >= rtiles) continue;
      const int j = jt * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * q + r, n = n0 + i;
        const bool in = n < N && j < Cr;
        const float v = in && h[(size_t)n * Cr + j] > 0.f ? acc[t][r] : 0.f;
        hl[i * ldh + j] = v;
        if (in) dz1[(size_t)n * Cr + j] = v;
      }
    }
  }
  __syncthreads();
  // ds = dz1 W1: B[k][c] = W1[k * C + c]
  fc_from_lds(hl, ldh, W1, (size_t)C, 1, ds, n0, N, C, Cr,
              [](float z, int) { return z; });
}

// One wave per 16 x 16 tile; grid ceil(2 * tiles / 4) blocks of four waves.
// Tiles [0, T): dW2 [C, Cr] = dz2^T h, then [T, 2T): dW1 [Cr, C] = dz1^T s.
__global__ __launch_bounds__(256)
void se_excite_wgrad_kernel(const float* __restrict__ dz2,
                            const float* __restrict__ h,
                            const float* __restrict__ dz1,
                            const float* __restrict__ s,
                            float* __restrict__ dW2, float* __restrict__ db2,
                            float* __restrict__ dW1, float* __restrict__ db1,
                            int N, int C, int Cr) {
  const int lane = threadIdx.x & 63, li = lane & 15, q = lane >> 4;
  const int T = ((C + 15) / 16) * ((Cr + 15) / 16);
  int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= 2 * T) return;   // a whole wave; the kernel has no barrier
  const bool first = t < T;
  if (!first) t -= T;
  const float* A = first ? dz2 : dz1;   // [N, rows]
  const float* B = first ? h : s;       // [N, cols]
  float* dW = first ? dW2 : dW1;        // [rows, cols]
  float* db = first ? db2 : db1;        // [rows]
  const int rows = first ? C : Cr, cols = first ? Cr : C;
  const int ctiles = (cols + 15) / 16;
  const int row = (t / ctiles) * 16 + li, col = (t % ctiles) * 16 + li;
  const bool bias = t % ctiles == 0;    // the same in all of a wave

  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  for (int nb = 0; nb < N; nb += 4 * GU) {   // GU steps' loads in flight
    float a[GU], b[GU];
#pragma unroll
    for (int gi = 0; gi < GU; ++gi) {
      const int n = nb + 4 * gi + q;           // past N: zeros
      a[gi] = (n < N && row < rows) ? A[(size_t)n * rows + row] : 0.f;
      b[gi] = (n < N && col < cols) ? B[(size_t)n * cols + col] : 0.f;
    }
#pragma unroll
    for (int gi = 0; gi < GU; ++gi) {
      acc = mfma4(a[gi], b[gi], acc);
      if (bias) accb = mfma4(a[gi], 1.f, accb);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = (t / ctiles) * 16 + 4 * q + r;
    if (i < rows && col < cols) dW[(size_t)i * cols + col] = acc[r];
    if (bias && li == 0 && i < rows) db[i] = accb[r];
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
hipStream_t se_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 ||
                              t.scalar_type() == at::kHalf),
              "se block: ", name, " must be a bf16 or fp16 HIP tensor, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.numel() > 0 &&
              t.is_contiguous(at::MemoryFormat::ChannelsLast),
              "se block: ", name, " must be 4-D channels_last");
  TORCH_CHECK(t.size(1) % 8 == 0, "se block: C must be a multiple of 8, got ",
              t.size(1));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "se block: ", name, " must be 16-byte aligned");
  TORCH_CHECK(t.numel() / 8 < (1L << 31) && t.size(1) < (1L << 22),
              "se block: ", name, " is too large (2^34 elements or 2^22 "
              "channels)");
}

inline void check_like(const at::Tensor& t, const char* name,
                       const at::Tensor& u) {
  check_act(t, name);
  TORCH_CHECK(t.scalar_type() == u.scalar_type() && t.sizes() == u.sizes(),
              "se block: ", name, " must have the dtype and shape of u, got ",
              t.scalar_type(), " ", t.sizes(), " for ", u.scalar_type(), " ",
              u.sizes());
}

inline void check_f32(const at::Tensor& t, const char* name,
                      at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
              t.is_contiguous(),
              "se block: ", name, " must be a contiguous fp32 HIP tensor, got ",
              t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, "se block: ", name, " must be ", shape,
              ", got ", t.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "se block: ", name, " must be 16-byte aligned");
}

inline void check_widths(long N, long C, long Cr) {
  TORCH_CHECK(N > 0 && C > 0 && C % 8 == 0 && C < (1L << 22),
              "se block: C must be a multiple of 8 below 2^22, got ", C);
  TORCH_CHECK(Cr >= 1 && Cr <= MAX_CR, "se block: the reduced width must be "
              "in 1..", MAX_CR, ", got ", Cr);
  TORCH_CHECK(N < (1L << 24), "se block: batch of 2^24 or more");
}

inline size_t excite_lds(long Cr) {
  return sizeof(float) * (MT * LDA + MT * (((Cr + 15) & ~15L) + 4));
}

template <typename T, bool BWD>
void launch_reduce(const at::Tensor& u, const at::Tensor* out,
                   const at::Tensor* dout, at::Tensor& dst, float scale) {
  const int N = u.size(0), C = u.size(1), HW = u.size(2) * u.size(3);
  const T* up = reinterpret_cast<const T*>(u.data_ptr());
  const T* op = BWD ? reinterpret_cast<const T*>(out->data_ptr()) : nullptr;
  const T* dp = BWD ? reinterpret_cast<const T*>(dout->data_ptr()) : nullptr;
  float* d = dst.data_ptr<float>();
  const int ni = HW <= 1 ? 32 : HW <= 4 ? 8 : HW <= 16 ? 2 : 1;
  const dim3 grid((N + ni - 1) / ni, (C + CHUNK - 1) / CHUNK);
#define SE_REDUCE(NI)                                                        \
  hipLaunchKernelGGL((se_reduce_kernel<T, NI, BWD>), grid, dim3(256), 0,     \
                     se_stream(), up, op, dp, d, N, C, HW, scale)
  if (ni == 32) SE_REDUCE(32);
  else if (ni == 8) SE_REDUCE(8);
  else if (ni == 2) SE_REDUCE(2);
  else SE_REDUCE(1);
#undef SE_REDUCE
}

}  // namespace

at::Tensor se_squeeze(at::Tensor u) {
  check_act(u, "u");
  auto s = at::empty({u.size(0), u.size(1)}, u.options().dtype(at::kFloat));
  const float scale = 1.f / (float)(u.size(2) * u.size(3));
  if (u.scalar_type() == at::kHalf)
    launch_reduce<_Float16, false>(u, nullptr, nullptr, s, scale);
  else
    launch_reduce<__bf16, false>(u, nullptr, nullptr, s, scale);
  return s;
}

std::tuple<at::Tensor, at::Tensor> se_excite_fwd(at::Tensor s, at::Tensor w1,
                                                 at::Tensor b1, at::Tensor w2,
                                                 at::Tensor b2) {
  TORCH_CHECK(s.dim() == 2 && w1.dim() == 2,
              "se block: s must be [N, C] and fc1.weight [Cr, C]");
  const long N = s.size(0), C = s.size(1), Cr = w1.size(0);
  check_widths(N, C, Cr);
  check_f32(s, "s", {N, C});
  check_f32(w1, "fc1.weight", {Cr, C});
  check_f32(b1, "fc1.bias", {Cr});
  check_f32(w2, "fc2.weight", {C, Cr});
  check_f32(b2, "fc2.bias", {C});
  auto h = at::empty({N, Cr}, s.options());
  auto g = at::empty({N, C}, s.options());
  hipLaunchKernelGGL(se_excite_fwd_kernel, dim3((N + MT - 1) / MT), dim3(256),
                     excite_lds(Cr), se_stream(), s.data_ptr<float>(),
                     w1.data_ptr<float>(), b1.data_ptr<float>(),
                     w2.data_ptr<float>(), b2.data_ptr<float>(),
                     h.data_ptr<float>(), g.data_ptr<float>(), (int)N, (int)C,
                     (int)Cr);
  return {h, g};
}

at::Tensor se_scale_add_relu(at::Tensor u, at::Tensor identity, at::Tensor g) {
  check_act(u, "u");
  check_like(identity, "identity", u);
  const long N = u.size(0), C = u.size(1), HW = u.size(2) * u.size(3);
  check_f32(g, "g", {N, C});
  auto out = at::empty_like(u);
  const unsigned nvec = (unsigned)(u.numel() / 8), C8 = (unsigned)(C / 8);
  const dim3 grid((nvec + 255) / 256);
  if (u.scalar_type() == at::kHalf)
    hipLaunchKernelGGL(se_scale_add_relu_kernel<_Float16>, grid, dim3(256), 0,
                       se_stream(),
                       reinterpret_cast<const _Float16*>(u.data_ptr()),
                       reinterpret_cast<const _Float16*>(identity.data_ptr()),
                       g.data_ptr<float>(),
                       reinterpret_cast<_Float16*>(out.data_ptr()), nvec, C8,
                       (unsigned)HW * C8);
  else
    hipLaunchKernelGGL(se_scale_add_relu_kernel<__bf16>, grid, dim3(256), 0,
                       se_stream(),
                       reinterpret_cast<const __bf16*>(u.data_ptr()),
                       reinterpret_cast<const __bf16*>(identity.data_ptr()),
                       g.data_ptr<float>(),
                       reinterpret_cast<__bf16*>(out.data_ptr()), nvec, C8,
                       (unsigned)HW * C8);
  return out;
}

at::Tensor se_join_bwd_reduce(at::Tensor dout, at::Tensor out, at::Tensor u) {
  check_act(u, "u");
  check_like(out, "out", u);
  check_like(dout, "dout", u);
  auto dg = at::empty({u.size(0), u.size(1)}, u.options().dtype(at::kFloat));
  if (u.scalar_type() == at::kHalf)
    launch_reduce<_Float16, true>(u, &out, &dout, dg, 1.f);
  else
    launch_reduce<__bf16, true>(u, &out, &dout, dg, 1.f);
  return dg;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> se_excite_bwd(
    at::Tensor dg, at::Tensor g, at::Tensor h, at::Tensor w1, at::Tensor w2) {
  TORCH_CHECK(dg.dim() == 2 && w1.dim() == 2,
              "se block: dg must be [N, C] and fc1.weight [Cr, C]");
  const long N = dg.size(0), C = dg.size(1), Cr = w1.size(0);
  check_widths(N, C, Cr);
  check_f32(dg, "dg", {N, C});
  check_f32(g, "g", {N, C});
  check_f32(h, "h", {N, Cr});
  check_f32(w1, "fc1.weight", {Cr, C});
  check_f32(w2, "fc2.weight", {C, Cr});
  auto dz2 = at::empty({N, C}, dg.options());
  auto dz1 = at::empty({N, Cr}, dg.options());
  auto ds = at::empty({N, C}, dg.options());
  hipLaunchKernelGGL(se_excite_bwd_kernel, dim3((N + MT - 1) / MT), dim3(256),
                     excite_lds(Cr), se_stream(), dg.data_ptr<float>(),
                     g.data_ptr<float>(), h.data_ptr<float>(),
                     w1.data_ptr<float>(), w2.data_ptr<float>(),
                     dz2.data_ptr<float>(), dz1.data_ptr<float>(),
                     ds.data_ptr<float>(), (int)N, (int)C, (int)Cr);
  return {dz2, dz1, ds};
}

// -> (dW1 [Cr, C], db1 [Cr], dW2 [C, Cr], db2 [C])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_excite_wgrad(
    at::Tensor dz2, at::Tensor h, at::Tensor dz1, at::Tensor s) {
  TORCH_CHECK(dz2.dim() == 2 && dz1.dim() == 2,
              "se block: dz2 must be [N, C] and dz1 [N, Cr]");
  const long N = dz2.size(0), C = dz2.size(1), Cr = dz1.size(1);
  check_widths(N, C, Cr);
  check_f32(dz2, "dz2", {N, C});
  check_f32(h, "h", {N, Cr});
  check_f32(dz1, "dz1", {N, Cr});
  check_f32(s, "s", {N, C});
  auto dW1 = at::empty({Cr, C}, s.options());
  auto db1 = at::empty({Cr}, s.options());
  auto dW2 = at::empty({C, Cr}, s.options());
  auto db2 = at::empty({C}, s.options());
  const long tiles = 2 * ((C + 15) / 16) * ((Cr + 15) / 16);
  hipLaunchKernelGGL(se_excite_wgrad_kernel, dim3((tiles + 3) / 4), dim3(256),
                     0, se_stream(), dz2.data_ptr<float>(),
                     h.data_ptr<float>(), dz1.data_ptr<float>(),
                     s.data_ptr<float>(), dW2.data_ptr<float>(),
                     db2.data_ptr<float>(), dW1.data_ptr<float>(),
                     db1.data_ptr<float>(), (int)N, (int)C, (int)Cr);
  return {dW1, db1, dW2, db2};
}

// -> (du, d_identity), both written in full
std::tuple<at::Tensor, at::Tensor> se_join_bwd_apply(at::Tensor dout,
                                                     at::Tensor out,
                                                     at::Tensor g,
                                                     at::Tensor ds) {
  check_act(out, "out");
  check_like(dout, "dout", out);
  const long N = out.size(0), C = out.size(1), HW = out.size(2) * out.size(3);
  check_f32(g, "g", {N, C});
  check_f32(ds, "ds", {N, C});
  auto du = at::empty_like(out);
  auto didn = at::empty_like(out);
  const unsigned nvec = (unsigned)(out.numel() / 8), C8 = (unsigned)(C / 8);
  const dim3 grid((nvec + 255) / 256);
  const float inv_hw = 1.f / (float)HW;
  if (out.scalar_type() == at::kHalf)
    hipLaunchKernelGGL(se_join_bwd_apply_kernel<_Float16>, grid, dim3(256), 0,
                       se_stream(),
                       reinterpret_cast<const _Float16*>(dout.data_ptr()),
                       reinterpret_cast<const _Float16*>(out.data_ptr()),
                       g.data_ptr<float>(), ds.data_ptr<float>(),
                       reinterpret_cast<_Float16*>(du.data_ptr()),
                       reinterpret_cast<_Float16*>(didn.data_ptr()), nvec, C8,
                       (unsigned)HW * C8, inv_hw);
  else
    hipLaunchKernelGGL(se_join_bwd_apply_kernel<__bf16>, grid, dim3(256), 0,
                       se_stream(),
                       reinterpret_cast<const __bf16*>(dout.data_ptr()),
                       reinterpret_cast<const __bf16*>(out.data_ptr()),
                       g.data_ptr<float>(), ds.data_ptr<float>(),
                       reinterpret_cast<__bf16*>(du.data_ptr()),
                       reinterpret_cast<__bf16*>(didn.data_ptr()), nvec, C8,
                       (unsigned)HW * C8, inv_hw);
  return {du, didn};
}
