// MI355X (gfx950/CDNA4) implicit-GEMM convolution kernels — NHWC bf16 or
// fp16 (every kernel that computes is templated on the element type, see
// Elem16; "bf16" in the comments below stands for either format).
//
// Replaces the reference's dependency on cuDNN conv kernels (SURVEY.md §2.2
// N1: 3x3 s1/s2 and 1x1 convs of the CIFAR ResNet, fwd + dgrad + wgrad).
// Written MFMA-first for CDNA4: v_mfma_f32_16x16x32_bf16 tiles, fp32
// accumulation, LDS-staged operand tiles sized for 64-wide wavefronts.
//
// GEMM views (all NHWC, reduction in fp32):
//   fwd  : out[N*P*Q][Kout] = im2col(x)[M][R*S*C]   @ w[Kout][R*S*C]^T
//   dgrad: dx[N*H*W][C]     = im2col'(dy)[M][R*S*K] @ wT[C][R*S*K]^T
//          (wT = weight rotated 180° and transposed to [C][R][S][K], built
//           host-side — a few KB)
//   wgrad: dw[Kout][R*S*C]  = dy^T[Kout][N*P*Q]     @ im2col(x)[N*P*Q][R*S*C]
//          (split-K over N*P*Q chunks, private fp32 partial slabs + reduce)
//
// FAST path: when the contiguous channel count is a multiple of BK(=64) a
// BK-sized reduction chunk lies inside ONE (r,s) filter tap with a contiguous
// channel run — every A-tile row is one 64-byte-aligned 128 B global read
// (or zero-fill). This covers every ResNet conv except the 3-channel stem.
//
// PADC path (the stem): C==3 inputs are padded once per call to 4 channels
// (x -> NHWC C=4; weight -> [K][K_pad] with K_pad = R*S*4 rounded up to BK,
// zero-filled), which makes every filter tap a naturally-aligned 8 B dwordx2
// gather — 4x fewer loads and ~8x less address math than the per-element
// generic gather that round 1 used for the stem.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <vector>

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

// The 16-bit element format of a kernel: __bf16 or _Float16. Staging, LDS
// layout, transposes and slabs move 16-bit patterns whatever they hold; the
// format decides only the x8 operand type, the MFMA instruction
// (v_mfma_f32_16x16x32_{bf16,f16}: same operand layout, 8 elements per lane
// for A and B, f32x4 for C/D) and the float -> element rounding. Both
// conversions are plain round-to-nearest-even; fp16 does not saturate: a
// value beyond 65504 becomes +-inf and NaN stays NaN, as in ATen and MIOpen,
// which is what a loss scaler's inf check relies on.
template <typename T> struct Elem16;

template <> struct Elem16<__bf16> {
  typedef __attribute__((ext_vector_type(8))) __bf16 x8;
  static __device__ __forceinline__ f32x4 mfma(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ __bf16 from_float(float v) {
    return (__bf16)v;
  }
};

template <> struct Elem16<_Float16> {
  typedef __attribute__((ext_vector_type(8))) _Float16 x8;
  static __device__ __forceinline__ f32x4 mfma(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ _Float16 from_float(float v) {
    return (_Float16)v;
  }
};

constexpr int BM = 128;   // GEMM M tile (output pixels)
constexpr int BN = 64;    // GEMM N tile (output channels / rsc)
constexpr int BK = 64;    // reduction tile
constexpr int LDK = BK + 8;  // padded LDS row stride: (m*LDK) covers all 64
                             // banks across a 16-lane ds_read_b128 group

struct ConvDims {
  int Nb;                // batch
  int OH, OW;            // spatial dims of the GEMM-M tensor (out / in)
  int GH, GW, GC;        // dims of the gathered tensor (x for fwd, dy for dgrad)
  int R, S;              // filter
  int stride, pad;
  int M, N, K;           // GEMM sizes: K = R*S*GC
};

// Decode a flat GEMM-M row into (image, row, col).
__device__ __forceinline__ void decode_m(int m, const ConvDims& d,
                                         int& n, int& oh, int& ow) {
  ow = m % d.OW;
  const int t = m / d.OW;
  oh = t % d.OH;
  n = t / d.OH;
}

// Input row coordinate for filter tap i. MODE 0 = fwd (oh is an output pixel,
// gather from x); MODE 1/2 = dgrad (oh is an input pixel, gather from dy with
// the transpose-conv index relation; tap index i is the 180°-rotated r).
// MODE 2 is the stride-2 parity-decomposed dgrad: each block handles one
// (h%2, w%2) output class, so filter taps whose divisibility test fails for
// the whole class are skipped wholesale (see the k-loop).
template <int MODE>
__device__ __forceinline__ bool tap_coord(int oh, int i, int filt, int stride,
                                          int pad, int lim, int& ih) {
  if (MODE == 0) {
    ih = oh * stride + i - pad;
    return ih >= 0 && ih < lim;
  }
  const int t = oh + pad - filt + 1 + i;
  if (t < 0 || t % stride != 0) return false;
  ih = t / stride;
  return ih < lim;
}

// MODE 2 row decode: class-local m -> real (n, oh, ow) for parity (pa, pb).
__device__ __forceinline__ void decode_m2(int m, const ConvDims& d,
                                          int pa, int pb,
                                          int& n, int& oh, int& ow) {
  const int ow2 = d.OW >> 1, oh2 = d.OH >> 1;
  ow = (m % ow2) * 2 + pb;
  const int t = m / ow2;
  oh = (t % oh2) * 2 + pa;
  n = t / oh2;
}

// ---------------------------------------------------------------------------
// fwd / dgrad kernel: out[M][N] = gatherA[M][K] @ B[N][K]^T
// 256 threads = 4 waves as a 2x2 wave grid; per wave 64x32 via 4x2 MFMA tiles.
// ---------------------------------------------------------------------------
// BMT = GEMM-M tile (128 default; 64 doubles the block count for the late
// small-M stages so they still fill 256 CUs). MI = BMT/32 MFMA row-tiles per
// wave; EPT = BMT/4 = A-tile elements each thread stages per BK chunk.
// PADC: gathered tensor has GC==4 (channel-padded stem); d.K is R*S*4 rounded
// up to BK and the B operand is the [N][d.K] zero-padded weight, so every
// A-tile tap is one aligned dwordx2 and every B row a pair of float4s.
// BNT = GEMM-N tile: 64 default; 128 halves the number of N-tiles — and
// with it the per-pass re-reads of the gathered A operand — for the wide-N
// high-C shapes (ResNet50's 1x1 expansions), where fwd/dgrad is A-traffic
// bound.
// SPLITK (FAST, MODE 0/1, 128x128 only): split-K for the small-M late stages,
// where 128x128 tiles alone leave most CUs without a block. blockIdx.z is the
// slice; slice z runs the pipelined K loop over its own contiguous range of
// BK tiles (balanced: ranges differ by at most one tile; the host keeps
// gridDim.z <= K / BK, so none is empty) and dumps its fp32 accumulators in
// fragment order into a private slab, as the wgrad kernels do (see
// store_frag_slab): `out` then points at the fp32 slabs, not at the 16-bit
// output. No atomics, no zero-init; igemm_reduce_frag_kernel sums the slices
// and rounds once.
template <int NF>
__device__ __forceinline__ void store_frag_slab(float* __restrict__ dwp,
                                                const f32x4* acc, int tid);

// BNEPI (MODE 0 only): the evaluation-mode epilogue. BatchNorm in eval mode
// is a per-channel affine map, so the conv applies it to the fp32 accumulator
// it still holds, adds the residual, clamps and rounds ONCE:
//   out = round(relu(fma(acc, scale[n], shift[n]) + res[m][n]))
// scale/shift are fp32 [N]; res is null or an [M][N] tensor of the output's
// dtype; fmaxf drops a NaN as bn_fwd_vec_kernel does. The plain kernels take
// an empty struct in its place and compile as they did without it.
struct NoEpi {};
template <typename T> struct BnEpi {
  const float* scale;
  const float* shift;
  const T* res;
  int relu;
};
template <typename T, bool BNEPI> struct EpiArg { typedef NoEpi type; };
template <typename T> struct EpiArg<T, true> { typedef BnEpi<T> type; };

template <typename T, int MODE, bool FAST, int BMT = BM, bool PADC = false,
          int BNT = BN, bool SPLITK = false, bool BNEPI = false>
__global__ __launch_bounds__(256)
void conv_igemm_kernel(const T* __restrict__ Ag,
                       const T* __restrict__ Bg,
                       T* __restrict__ out, ConvDims d,
                       typename EpiArg<T, BNEPI>::type ep) {
  static_assert(!SPLITK || (FAST && MODE != 2 && !PADC && BMT == 128 &&
                            BNT == 128),
                "split-K exists for the pipelined 128x128 tile only");
  static_assert(!BNEPI || (MODE == 0 && !SPLITK),
                "the BN epilogue is a forward epilogue; split-K applies it in "
                "the reduce");
  typedef typename Elem16<T>::x8 x8;
  constexpr int MI = BMT / 32;
  constexpr int NI = BNT / 32;
  constexpr int EPT = BMT / 4;          // 32 or 16 elems per loader thread
  constexpr int PER_ROW = 64 / EPT;     // loader threads per A row
  constexpr int BEPT = BK * BNT / 256;  // B elems per loader thread
  __shared__ T sA[BMT * LDK];
  __shared__ T sB[BNT * LDK];

  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * BMT;
  const int n0 = blockIdx.x * BNT;
  const int pa = (MODE == 2) ? (int)(blockIdx.z & 1) : 0;
  const int pb = (MODE == 2) ? (int)(blockIdx.z >> 1) : 0;

  // A loader: thread -> (row, EPT-element slice of the BK chunk)
  const int a_row = tid / PER_ROW;
  const int a_off = (tid % PER_ROW) * EPT;
  int a_n, a_oh, a_ow;
  {
    int m = m0 + a_row;
    if (m >= d.M) m = d.M - 1;  // clamped rows only feed predicated-out outputs
    if (MODE == 2) decode_m2(m, d, pa, pb, a_n, a_oh, a_ow);
    else decode_m(m, d, a_n, a_oh, a_ow);
  }
  // B loader: thread -> (row, BEPT-element slice of the BK chunk)
  const int b_row = tid & (BNT - 1);
  const int b_off = (tid / BNT) * BEPT;
  const long b_base = (long)min(n0 + b_row, d.N - 1) * d.K;

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * (BMT / 2);
  const int wn = (wave & 1) * (BNT / 2);
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;

  f32x4 acc[MI][NI] = {};

  const int SC = d.S * d.GC;

  // ---- FAST-path staging helpers (explicit scalars: an array here is
  // demoted to scratch — an 80 B/lane spill measured 2-3x on the kernel) ----
  auto issue_A = [&](int kk0, float4& v0, float4& v1, float4& v2, float4& v3) {
    const int i = kk0 / SC;
    const int rem = kk0 - i * SC;
    const int j = rem / d.GC;
    const int c0 = rem - j * d.GC + a_off;
    int ih, iw;
    const bool ok = tap_coord<MODE>(a_oh, i, d.R, d.stride, d.pad, d.GH, ih)
                  & tap_coord<MODE>(a_ow, j, d.S, d.stride, d.pad, d.GW, iw);
    v0 = v1 = v2 = v3 = float4{};
    if (ok) {
      const float4* src = (const float4*)(Ag +
          (((long)a_n * d.GH + ih) * d.GW + iw) * d.GC + c0);
      v0 = src[0];
      v1 = src[1];
      if constexpr (EPT == 32) {
        v2 = src[2];
        v3 = src[3];
      }
    }
  };
  auto write_A = [&](float4 v0, float4 v1, float4 v2, float4 v3) {
    float4* dst = (float4*)(sA + a_row * LDK + a_off);
    dst[0] = v0;
    dst[1] = v1;
    if constexpr (EPT == 32) {
      dst[2] = v2;
      dst[3] = v3;
    }
  };
  // explicit scalar refs, NOT an array or struct: anything indexable (or
  // aggregate) here is demoted to scratch — the r2c3 BNT refactor's
  // float4[] cost the pipelined kernels ~1.6x (144 B/lane spill)
  auto issue_B = [&](int kk0, float4& v0, float4& v1, float4& v2, float4& v3) {
    const float4* src = (const float4*)(Bg + b_base + kk0 + b_off);
    v0 = src[0];
    v1 = src[1];
    if constexpr (BEPT == 32) {
      v2 = src[2];
      v3 = src[3];
    }
  };
  auto write_B = [&](float4 v0, float4 v1, float4 v2, float4 v3) {
    float4* dst = (float4*)(sB + b_row * LDK + b_off);
    dst[0] = v0;
    dst[1] = v1;
    if constexpr (BEPT == 32) {
      dst[2] = v2;
      dst[3] = v3;
    }
  };
  auto mfma_tile = [&]() {
    #pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      x8 af[MI], bf[NI];
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        af[mi] = *(const x8*)&sA[(wm + mi * 16 + fr) * LDK + ks + fk];
      #pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        bf[ni] = *(const x8*)&sB[(wn + ni * 16 + fr) * LDK + ks + fk];
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = Elem16<T>::mfma(af[mi], bf[ni], acc[mi][ni]);
    }
  };

  if constexpr (PADC) {
    const int RS = d.R * d.S;
    for (int kk0 = 0; kk0 < d.K; kk0 += BK) {
      // A tile: one aligned 8 B dwordx2 per filter tap (4 padded channels)
      #pragma unroll
      for (int e = 0; e < EPT / 4; ++e) {
        const int t4 = a_off + e * 4;
        const int tap = (kk0 + t4) >> 2;
        float2 v = {};
        if (tap < RS) {
          const int i = tap / d.S, j = tap - (tap / d.S) * d.S;
          int ih, iw;
          if (tap_coord<MODE>(a_oh, i, d.R, d.stride, d.pad, d.GH, ih) &&
              tap_coord<MODE>(a_ow, j, d.S, d.stride, d.pad, d.GW, iw))
            v = *(const float2*)(Ag +
                (((long)a_n * d.GH + ih) * d.GW + iw) * 4);
        }
        *(float2*)(sA + a_row * LDK + t4) = v;
      }
      // B tile: rows are d.K-long (BK multiple) -> always-aligned float4s
      {
        float4 b0, b1, b2, b3;
        issue_B(kk0, b0, b1, b2, b3);
        write_B(b0, b1, b2, b3);
      }
      __syncthreads();
      mfma_tile();
      __syncthreads();
    }
  } else if constexpr (FAST && MODE != 2) {
    // Register-pipelined: tile k+1's global loads issue before tile k's
    // MFMAs, so HBM/L2 latency overlaps compute; the waits land at the LDS
    // write after the barrier (write-after-barrier form).
    int kbeg = 0, kend = d.K;
    if constexpr (SPLITK) {
      // slice z of S takes tiles [z*q + min(z, r), +q + (z < r)), q = T / S,
      // r = T % S: the first r slices are one tile longer
      const int nkt = d.K / BK, S = (int)gridDim.z, z = (int)blockIdx.z;
      const int q = nkt / S, r = nkt - q * S;
      const int t0 = z * q + min(z, r);
      kbeg = t0 * BK;
      kend = (t0 + q + (z < r ? 1 : 0)) * BK;
    }
    {
      float4 a0, a1, a2, a3, b0, b1, b2, b3;
      issue_A(kbeg, a0, a1, a2, a3);
      issue_B(kbeg, b0, b1, b2, b3);
      write_A(a0, a1, a2, a3);
      write_B(b0, b1, b2, b3);
    }
    __syncthreads();
    for (int kk0 = kbeg; kk0 < kend; kk0 += BK) {
      const bool has_next = kk0 + BK < kend;
      float4 a0 = {}, a1 = {}, a2 = {}, a3 = {};
      float4 b0 = {}, b1 = {}, b2 = {}, b3 = {};
      if (has_next) {
        issue_A(kk0 + BK, a0, a1, a2, a3);
        issue_B(kk0 + BK, b0, b1, b2, b3);
      }
      mfma_tile();
      if (has_next) {
        __syncthreads();
        write_A(a0, a1, a2, a3);
        write_B(b0, b1, b2, b3);
        __syncthreads();
      }
    }
  } else {
    for (int kk0 = 0; kk0 < d.K; kk0 += BK) {
      // ---- stage A tile ---------------------------------------------
      if (FAST) {  // MODE == 2 only (other FAST modes take the pipeline)
        if (MODE == 2) {
          // stride-2 divisibility is class-uniform: skip the whole tap when
          // either axis has the wrong parity (3/4 of taps for 3x3 s2 dgrad)
          const int i = kk0 / SC;
          const int rem = kk0 - i * SC;
          const int j = rem / d.GC;
          const int ta = pa + d.pad - d.R + 1 + i;
          const int tb = pb + d.pad - d.S + 1 + j;
          if ((ta & 1) || (tb & 1)) continue;
        }
        float4 a0, a1, a2, a3, b0, b1, b2, b3;
        issue_A(kk0, a0, a1, a2, a3);
        issue_B(kk0, b0, b1, b2, b3);
        write_A(a0, a1, a2, a3);
        write_B(b0, b1, b2, b3);
      } else {
        // generic gather: one element at a time (stem conv only)
        for (int e = tid; e < BMT * BK; e += 256) {
          const int row = e >> 6, kk = kk0 + (e & 63);
          T v = (T)0.f;
          if (kk < d.K) {
            int m = m0 + row;
            if (m >= d.M) m = d.M - 1;
            int n, oh, ow;
            decode_m(m, d, n, oh, ow);
            const int i = kk / SC, rem = kk - i * SC;
            const int j = rem / d.GC, c = rem - j * d.GC;
            int ih, iw;
            if (tap_coord<MODE>(oh, i, d.R, d.stride, d.pad, d.GH, ih) &&
                tap_coord<MODE>(ow, j, d.S, d.stride, d.pad, d.GW, iw))
              v = Ag[(((long)n * d.GH + ih) * d.GW + iw) * d.GC + c];
          }
          sA[row * LDK + (e & 63)] = v;
        }
        for (int e = tid; e < BNT * BK; e += 256) {
          const int row = e >> 6, kk = kk0 + (e & 63);
          sB[row * LDK + (e & 63)] = (kk < d.K)
              ? Bg[(long)min(n0 + row, d.N - 1) * d.K + kk] : (T)0.f;
        }
      }
      __syncthreads();
      mfma_tile();
      __syncthreads();
    }
  }

  if constexpr (SPLITK) {
    // edge tiles included: rows / columns past M / N hold what the clamped
    // loads accumulated and are dropped by the reduce
    store_frag_slab<MI * NI>(reinterpret_cast<float*>(out), &acc[0][0], tid);
    return;
  }

  // ---- epilogue: D row = (lane>>4)*4 + reg, col = lane&15 ----------------
  const int dm = (lane >> 4) * 4;
  const int dn = lane & 15;
  // BNEPI: a lane's column is fixed per N-tile, so its two coefficients load
  // once per N-tile here (a column past N reads the last one and stores
  // nothing)
  float sc[BNEPI ? NI : 1], sh[BNEPI ? NI : 1];
  if constexpr (BNEPI) {
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = min(n0 + wn + ni * 16 + dn, d.N - 1);
      sc[ni] = ep.scale[n];
      sh[ni] = ep.shift[n];
    }
  }
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = n0 + wn + ni * 16 + dn;
      if (n >= d.N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + dm + r;
        if (m >= d.M) continue;
        long om = m;
        if (MODE == 2) {
          int on, ooh, oow;
          decode_m2(m, d, pa, pb, on, ooh, oow);
          om = ((long)on * d.OH + ooh) * d.OW + oow;
        }
        if constexpr (BNEPI) {
          float v = fmaf(acc[mi][ni][r], sc[ni], sh[ni]);
          if (ep.res != nullptr) v += (float)ep.res[om * d.N + n];
          if (ep.relu) v = fmaxf(v, 0.f);
          out[om * d.N + n] = Elem16<T>::from_float(v);
        } else {
          out[om * d.N + n] = Elem16<T>::from_float(acc[mi][ni][r]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad kernel: dw[Kout][RSC] += dy^T[Kout][NPQ-chunk] @ im2col(x)[chunk][RSC]
// 64x64 output tile per block, 2x2 waves of 32x32; split-K over NPQ chunks.
// Each grid.z slice accumulates ITS chunks in registers and stores a private
// fp32 partial slab (no atomics — round 1's fp32 atomicAdd contention was the
// main wgrad cost at small tm*tn); a reduce kernel sums the slabs and
// emits the bf16 channels_last weight grad in one pass. Slices beyond one
// resident set of blocks (CUs x blocks per CU) add slab traffic, not
// parallelism: splits < 0 asks for exactly that set. DIRECT (splits==1,
// no channel padding): the slab and reduce collapse away — the kernel writes
// bf16 dw itself. Both LDS tiles are written transposed (reduction index
// contiguous per row) so MFMA fragment reads are 16-byte ds_read_b128.
// PADC: x has 4 padded channels (stem) — per-tap dwordx2 gathers.
// ---------------------------------------------------------------------------
// ATOMIC: all grid.z slices atomicAdd into ONE fp32 slab (round 1's scheme)
// instead of private slabs — wins on small dw where the slab+reduce pass
// costs more than the contention; kept as autotune variant wtile=4.
//
// Partial-slab layout. The ATOMIC slab is row-major [m][n] and goes through
// wgrad_reduce_kernel. Every other split-K launch (v1 with the stem, v2,
// LIN) stores FRAGMENT-ORDER slabs
//   part[z][tile][f][tid] of f32x4,  tile = blockIdx.y * gridDim.x + blockIdx.x,
// where f = mi * 4 + ni walks the block's accumulator array and tid is the
// thread: the block dumps its registers as they are, one 16-byte store per
// lane per fragment, a wave covering 1 KiB contiguous (row-major cost one
// dword store per accumulator ELEMENT, four 64-byte pieces per wave
// instruction). A tile's region is TM*TN floats, edge tiles included: their
// out-of-range rows/columns are stored as accumulated and dropped by
// wgrad_reduce_frag_kernel, which undoes the permutation.
// Every dw element leaves through here. The value is rounded to the element
// format T either way; f32 stores that rounded value widened (exact), for an
// fp32 parameter whose gradient would otherwise be widened by a separate cast
// kernel. An fp16 overflow therefore arrives as inf in the fp32 gradient too.
template <typename T>
__device__ __forceinline__ void store_dw(void* __restrict__ dw, bool f32,
                                         long idx, float v) {
  const T b = Elem16<T>::from_float(v);
  if (f32) ((float*)dw)[idx] = (float)b;
  else ((T*)dw)[idx] = b;
}

template <int NF>
__device__ __forceinline__ void store_frag_slab(float* __restrict__ dwp,
                                                const f32x4* acc, int tid) {
  const long ntiles = (long)gridDim.x * gridDim.y;
  const long tile = (long)blockIdx.y * gridDim.x + blockIdx.x;
  f32x4* dst = (f32x4*)dwp + (blockIdx.z * ntiles + tile) * (NF * 256) + tid;
  #pragma unroll
  for (int f = 0; f < NF; ++f) dst[f * 256] = acc[f];
}

template <typename T, bool FAST, bool PADC = false, bool DIRECT = false,
          bool ATOMIC = false>
__global__ __launch_bounds__(256)
void conv_wgrad_kernel(const T* __restrict__ dy,
                       const T* __restrict__ x,
                       float* __restrict__ dwp,
                       void* __restrict__ dwb, ConvDims d, bool f32) {
  typedef typename Elem16<T>::x8 x8;
  // d: M = Kout, N = R*S*C, K = Nb*P*Q; OH/OW = P,Q; GH/GW/GC = H,W,C
  // 64(Kout) x 128(rsc) tile: each loaded byte feeds twice the MFMA work of
  // the 64x64 tile. FAST needs C % 64 == 0 so every 32-wide rsc sub-chunk
  // stays inside one (r,s) filter tap.
  __shared__ T sA[64 * LDK];   // [kout][npq]
  __shared__ T sB[128 * LDK];  // [rsc][npq]

  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * 64;
  const int n0 = blockIdx.x * 128;
  const int row = tid & 63;        // npq row within the chunk
  const int grp = tid >> 6;        // 0..3

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 32;
  const int wn = (wave & 1) * 64;
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;

  const int SC = d.S * d.GC;
  const int nchunks = (d.K + BK - 1) / BK;
  f32x4 acc[2][4] = {};

  for (int kc = blockIdx.z; kc < nchunks; kc += gridDim.z) {
    const int kk0 = kc * BK;
    const int npq = kk0 + row;
    int xn, xp, xq;
    decode_m(min(npq, d.K - 1), d, xn, xp, xq);
    const bool npq_ok = npq < d.K;

    // ---- dy tile, transposed into sA[kout][npq] ------------------------
    {
      const int cg = grp * 16;
      T vals[16];
      // the row bound also guards FAST: K % 16 == 0 admits K % 64 != 0
      // (e.g. K=80 via the public conv2d API), where the last tile's 16-wide
      // float4 loads would run past dy
      if (npq_ok && m0 + cg + 16 <= d.M) {
        const float4* src = (const float4*)(dy + (long)npq * d.M + m0 + cg);
        *(float4*)&vals[0] = src[0];
        *(float4*)&vals[8] = src[1];
      } else {
        #pragma unroll
        for (int e = 0; e < 16; ++e)
          vals[e] = (npq_ok && m0 + cg + e < d.M)
              ? dy[(long)npq * d.M + m0 + cg + e] : (T)0.f;
      }
      #pragma unroll
      for (int e = 0; e < 16; ++e)
        sA[(cg + e) * LDK + row] = vals[e];
    }
    // ---- x tile (128 rsc cols = 4 x 32-col sub-chunks), transposed -----
    {
      const int cg = grp * 32;     // this thread's 32-col sub-chunk
      T vals[32];
      if (PADC) {
        // stem: 8 taps of 4 padded channels each, aligned dwordx2 gathers
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int nn = n0 + cg + e * 4;
          float2 v = {};
          if (npq_ok && nn < d.N) {
            const int tap = nn >> 2;
            const int i = tap / d.S, j = tap - (tap / d.S) * d.S;
            const int ih = xp * d.stride + i - d.pad;
            const int iw = xq * d.stride + j - d.pad;
            if (ih >= 0 && ih < d.GH && iw >= 0 && iw < d.GW)
              v = *(const float2*)(x +
                  (((long)xn * d.GH + ih) * d.GW + iw) * 4);
          }
          *(float2*)&vals[e * 4] = v;
        }
      } else if (FAST) {
        const int nn = n0 + cg;
        const int i = nn / SC;
        const int rem = nn - i * SC;
        const int j = rem / d.GC;
        const int c0 = rem - j * d.GC;
        const int ih = xp * d.stride + i - d.pad;
        const int iw = xq * d.stride + j - d.pad;
        if (npq_ok && ih >= 0 && ih < d.GH && iw >= 0 && iw < d.GW) {
          const float4* src = (const float4*)(x +
              (((long)xn * d.GH + ih) * d.GW + iw) * d.GC + c0);
          *(float4*)&vals[0] = src[0];
          *(float4*)&vals[8] = src[1];
          *(float4*)&vals[16] = src[2];
          *(float4*)&vals[24] = src[3];
        } else {
          #pragma unroll
          for (int e = 0; e < 32; ++e) vals[e] = (T)0.f;
        }
      } else {
        #pragma unroll
        for (int e = 0; e < 32; ++e) {
          const int nn = n0 + cg + e;
          T v = (T)0.f;
          if (npq_ok && nn < d.N) {
            const int i = nn / SC, rem = nn - i * SC;
            const int j = rem / d.GC, c = rem - j * d.GC;
            const int ih = xp * d.stride + i - d.pad;
            const int iw = xq * d.stride + j - d.pad;
            if (ih >= 0 && ih < d.GH && iw >= 0 && iw < d.GW)
              v = x[(((long)xn * d.GH + ih) * d.GW + iw) * d.GC + c];
          }
          vals[e] = v;
        }
      }
      #pragma unroll
      for (int e = 0; e < 32; ++e)
        sB[(cg + e) * LDK + row] = vals[e];
    }
    __syncthreads();

    #pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      x8 af[2], bf[4];
      #pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        af[mi] = *(const x8*)&sA[(wm + mi * 16 + fr) * LDK + ks + fk];
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bf[ni] = *(const x8*)&sB[(wn + ni * 16 + fr) * LDK + ks + fk];
      #pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = Elem16<T>::mfma(af[mi], bf[ni], acc[mi][ni]);
    }
    __syncthreads();
  }

  if constexpr (!DIRECT && !ATOMIC) {
    store_frag_slab<8>(dwp, &acc[0][0], tid);
    return;
  }
  const int dm = (lane >> 4) * 4;
  const int dn = lane & 15;
  float* slab = DIRECT ? nullptr
              : dwp + (ATOMIC ? 0L : (long)blockIdx.z * d.M * d.N);
  #pragma unroll
  for (int mi = 0; mi < 2; ++mi)
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + ni * 16 + dn;
      if (n >= d.N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + dm + r;
        if (m >= d.M) continue;
        if (DIRECT) store_dw<T>(dwb, f32, (long)m * d.N + n, acc[mi][ni][r]);
        else if (ATOMIC) atomicAdd(&slab[(long)m * d.N + n], acc[mi][ni][r]);
        else slab[(long)m * d.N + n] = acc[mi][ni][r];
      }
    }
}

// ---------------------------------------------------------------------------
// wgrad v2: large-tile variant for the big-spatial / big-channel shapes
// (ResNet50 @ 224px). Tile = (WGM*64) x (WGN*64) per 256-thread block
// ((2,2) -> 128x128, (4,1) -> 256x64): fewer K-passes over dy/x than v1's
// 64x128 (cross-tile re-reads scale with tile count), and the LDS transpose
// is done 4x4 in REGISTERS (8 v_perm per block) with ds_write_b64 stores —
// v1 staged with 48 scalar b16 LDS writes per thread per chunk, which
// rivalled the MFMA issue time. FAST-path shapes only (C % 64 == 0).
// ---------------------------------------------------------------------------

// transpose a 4x4 bf16 block: in[i] = row i as uint2 {e[i][0..1], e[i][2..3]},
// out[c] = column c. 8 v_perm_b32: selector picks [b0,b1,a0,a1]/[b2,b3,a2,a3]
// bytes of the {src1(b) low, src0(a) high} concatenation.
__device__ __forceinline__ void tr4x4_bf16(const uint2 in[4], uint2 out[4]) {
  const unsigned LO = 0x05040100u, HI = 0x07060302u;
  out[0].x = __builtin_amdgcn_perm(in[1].x, in[0].x, LO);
  out[0].y = __builtin_amdgcn_perm(in[3].x, in[2].x, LO);
  out[1].x = __builtin_amdgcn_perm(in[1].x, in[0].x, HI);
  out[1].y = __builtin_amdgcn_perm(in[3].x, in[2].x, HI);
  out[2].x = __builtin_amdgcn_perm(in[1].y, in[0].y, LO);
  out[2].y = __builtin_amdgcn_perm(in[3].y, in[2].y, LO);
  out[3].x = __builtin_amdgcn_perm(in[1].y, in[0].y, HI);
  out[3].y = __builtin_amdgcn_perm(in[3].y, in[2].y, HI);
}

// CH = BK-chunks per pipeline stage. CH=2 stages 128 npq rows so the MFMA
// phase (~64 MFMAs/wave, ~1100 cyc) covers the ~900-cyc load latency that
// left CH=1 at 54-57% SQ_WAIT_ANY (profiles/r2c13): LDS doubles (69.6 KB
// for (2,2) -> 2 blocks/CU) and staging registers double, trading
// block-level overlap for complete within-wave latency cover.
template <typename T, int WGM, int WGN, bool DIRECT, int CH = 1>
__global__ __launch_bounds__(256, 2)
void conv_wgrad_v2_kernel(const T* __restrict__ dy,
                          const T* __restrict__ x,
                          float* __restrict__ dwp,
                          void* __restrict__ dwb, ConvDims d, bool f32) {
  typedef typename Elem16<T>::x8 x8;
  constexpr int TM = WGM * 64;          // kout tile
  constexpr int TN = WGN * 64;          // rsc tile
  constexpr int TA = TM / 64;
  constexpr int TB = TN / 64;
  constexpr int SK = CH * BK;           // npq rows per stage
  constexpr int SLDK = SK + 8;          // padded LDS row length
  __shared__ T sA[TM * SLDK];      // [kout][npq]
  __shared__ T sB[TN * SLDK];      // [rsc][npq]
  // DOUBLE-BUFFERED per-chunk row metadata: for npq row r, the x base
  // offset of tap (0,0), the (ih0, iw0) coords for bounds tests, and a
  // validity flag (NOT derived from the offset sign — that offset is
  // legitimately negative for pad-boundary rows of image 0). Buffer b
  // holds the NEXT chunk's rows so its gathers can issue before the
  // current chunk's MFMAs (register pipeline, as in the LIN kernel).
  __shared__ int sRowOff[2][SK];        // (xn*GH + ih0)*GW + iw0
  __shared__ short sIh0[2][SK], sIw0[2][SK];
  __shared__ unsigned char sOk[2][SK];  // npq < d.K

  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * TM;
  const int n0 = blockIdx.x * TN;

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave / WGN) * 64;
  const int wn = (wave % WGN) * 64;
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;

  const int SC = d.S * d.GC;
  const int nstages = (d.K + SK - 1) / SK;
  f32x4 acc[4][4] = {};

  uint2 sta[TA * CH][4], stb[TB * CH][4];  // staged 4x4 blocks for one stage

  auto compute_meta = [&](int kc, int b) {
    if (tid < SK) {
      const int npq = kc * SK + tid;
      int off = 0, ih0 = 0, iw0 = 0;
      const bool ok = npq < d.K && kc < nstages;
      if (ok) {
        int xn, xp, xq;
        decode_m(npq, d, xn, xp, xq);
        ih0 = xp * d.stride - d.pad;
        iw0 = xq * d.stride - d.pad;
        off = ((xn * d.GH + ih0) * d.GW + iw0);
      }
      sRowOff[b][tid] = off;
      sIh0[b][tid] = (short)ih0;
      sIw0[b][tid] = (short)iw0;
      sOk[b][tid] = ok;
    }
  };
  // thread -> 4x4 block mapping is COLUMN-group-fastest so a wave's global
  // loads are contiguous; the transposed b64 stores are XOR-swizzled on the
  // npq quad (even bits only — 8-element fragment reads stay intact).
  auto issue_all = [&](int kk0, int b) {
    #pragma unroll
    for (int t = 0; t < TA * CH; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TM / 4 - 1);
      const int r4 = bid / (TM / 4);    // 0 .. 16*CH-1
      const int npq0 = kk0 + r4 * 4;
      const int mcol = m0 + c4 * 4;
      if (npq0 + 4 <= d.K && mcol + 4 <= d.M) {
        #pragma unroll
        for (int i = 0; i < 4; ++i)
          sta[t][i] = *(const uint2*)(dy + (long)(npq0 + i) * d.M + mcol);
      } else {
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
          T e[4] = {};
          if (npq0 + i < d.K)
            #pragma unroll
            for (int c = 0; c < 4; ++c)
              if (mcol + c < d.M)
                e[c] = dy[(long)(npq0 + i) * d.M + mcol + c];
          sta[t][i] = *(uint2*)e;
        }
      }
    }
    #pragma unroll
    for (int t = 0; t < TB * CH; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TN / 4 - 1);
      const int r4 = bid / (TN / 4);
      const int nn = n0 + c4 * 4;       // rsc col of this 4-col group
      // FAST contract (C % 64 == 0): nn..nn+3 sit inside ONE filter tap
      const int i_tap = nn / SC;
      const int rem = nn - i_tap * SC;
      const int j_tap = rem / d.GC;
      const int cch = rem - j_tap * d.GC;
      const bool ncol_ok = nn + 4 <= d.N;
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = r4 * 4 + i;
        uint2 v = {0u, 0u};
        if (ncol_ok && sOk[b][r]) {
          const int ih = sIh0[b][r] + i_tap;
          const int iw = sIw0[b][r] + j_tap;
          if (ih >= 0 && ih < d.GH && iw >= 0 && iw < d.GW)
            v = *(const uint2*)(x +
                ((long)sRowOff[b][r] + i_tap * d.GW + j_tap) * d.GC + cch);
        }
        stb[t][i] = v;
      }
    }
  };
  // swizzle note: q ranges over 16*CH quads; the XOR touches only bits 1-3
  // (even, <16), so swizzled quads stay inside their row for any CH
  auto write_all = [&]() {
    #pragma unroll
    for (int t = 0; t < TA * CH; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TM / 4 - 1);
      const int r4 = bid / (TM / 4);
      uint2 out[4];
      tr4x4_bf16(sta[t], out);
      const int q = r4 ^ (c4 & 14);
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        *(uint2*)(sA + (c4 * 4 + i) * SLDK + q * 4) = out[i];
    }
    #pragma unroll
    for (int t = 0; t < TB * CH; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TN / 4 - 1);
      const int r4 = bid / (TN / 4);
      uint2 out[4];
      tr4x4_bf16(stb[t], out);
      const int q = r4 ^ (c4 & 14);
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        *(uint2*)(sB + (c4 * 4 + i) * SLDK + q * 4) = out[i];
    }
  };
  auto mfma_all = [&]() {
    #pragma unroll
    for (int ks = 0; ks < SK; ks += 32) {
      x8 af[4], bf[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int row = wm + mi * 16 + fr;
        const int q = ((ks + fk) >> 2) ^ ((row >> 2) & 14);
        af[mi] = *(const x8*)&sA[row * SLDK + q * 4];
      }
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int row = wn + ni * 16 + fr;
        const int q = ((ks + fk) >> 2) ^ ((row >> 2) & 14);
        bf[ni] = *(const x8*)&sB[row * SLDK + q * 4];
      }
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = Elem16<T>::mfma(af[mi], bf[ni], acc[mi][ni]);
    }
  };

  // pipeline: meta(k) -> loads(k) -> tiles(k); then per chunk k:
  //   loads(k+1) [covered by MFMA(k)] / MFMA(k) / write tiles(k+1) +
  //   meta(k+2) between two barriers
  bool first = true;
  int buf = 0;
  for (int kc = blockIdx.z; kc < nstages; kc += gridDim.z) {
    const int kn = kc + gridDim.z;
    if (first) {
      compute_meta(kc, 0);
      __syncthreads();
      issue_all(kc * SK, 0);
      write_all();
      compute_meta(kn, 1);
      __syncthreads();
      first = false;
      buf = 1;                          // meta[1] holds stage kn
    }
    const bool has_next = kn < nstages;
    if (has_next) issue_all(kn * SK, buf);
    mfma_all();
    if (has_next) {
      __syncthreads();
      write_all();
      compute_meta(kn + gridDim.z, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  if constexpr (!DIRECT) {
    store_frag_slab<16>(dwp, &acc[0][0], tid);
    return;
  }
  const int dm = (lane >> 4) * 4;
  const int dn = lane & 15;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + ni * 16 + dn;
      if (n >= d.N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + dm + r;
        if (m >= d.M) continue;
        store_dw<T>(dwb, f32, (long)m * d.N + n, acc[mi][ni][r]);
      }
    }
}

// ---------------------------------------------------------------------------
// wgrad v3 (LIN): 1x1 stride-1 pad-0 shapes — the bulk of ResNet50's wgrad
// time. im2col(x) IS x, so BOTH operands are plain row-major [npq][C]:
// no gather, no row metadata, and the whole chunk pipeline can be
// register-double-buffered like the fwd kernel (loads for chunk k+1 issue
// before chunk k's MFMAs, hiding the ~900-cycle HBM latency that left v2 at
// ~38% of peak bandwidth). Tile = (WGM*64) x (WGN*64), 2 barriers/chunk.
// ---------------------------------------------------------------------------
template <typename T, int WGM, int WGN, bool DIRECT>
__global__ __launch_bounds__(256, 2)  // 2 waves/SIMD: the double buffer
                                      // needs a partner wave per SIMD
void conv_wgrad_lin_kernel(const T* __restrict__ dy,
                           const T* __restrict__ x,
                           float* __restrict__ dwp,
                           void* __restrict__ dwb, ConvDims d, bool f32) {
  typedef typename Elem16<T>::x8 x8;
  constexpr int TM = WGM * 64;
  constexpr int TN = WGN * 64;
  constexpr int TA = TM / 64;
  constexpr int TB = TN / 64;
  __shared__ T sA[TM * LDK];
  __shared__ T sB[TN * LDK];

  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * TM;
  const int n0 = blockIdx.x * TN;

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave / WGN) * 64;
  const int wn = (wave % WGN) * 64;
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;

  const int nchunks = (d.K + BK - 1) / BK;
  f32x4 acc[4][4] = {};

  // staged 4x4 blocks for one chunk: [block][row] uint2, fully unrolled
  // (verify ScratchSize stays 0 — indexable locals here have spilled before)
  uint2 sta[TA][4], stb[TB][4];

  // per-pass block decomposition (c4-fastest => coalesced loads)
  auto load_op = [&](const T* src, int ncols, int c4n, int base,
                     int kk0, int bid, uint2 (&in)[4]) {
    const int c4 = bid & (c4n - 1);
    const int r4 = bid / c4n;
    const int row0 = kk0 + r4 * 4;
    const int col = base + c4 * 4;
    if (row0 + 4 <= d.K && col + 4 <= ncols) {
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        in[i] = *(const uint2*)(src + (long)(row0 + i) * ncols + col);
    } else {
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        T e[4] = {};
        if (row0 + i < d.K)
          #pragma unroll
          for (int c = 0; c < 4; ++c)
            if (col + c < ncols) e[c] = src[(long)(row0 + i) * ncols + col + c];
        in[i] = *(uint2*)e;
      }
    }
  };
  auto issue_all = [&](int kk0) {
    #pragma unroll
    for (int t = 0; t < TA; ++t)
      load_op(dy, d.M, TM / 4, m0, kk0, t * 256 + tid, sta[t]);
    #pragma unroll
    for (int t = 0; t < TB; ++t)
      load_op(x, d.N, TN / 4, n0, kk0, t * 256 + tid, stb[t]);
  };
  auto write_all = [&]() {
    #pragma unroll
    for (int t = 0; t < TA; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TM / 4 - 1);
      const int r4 = bid / (TM / 4);
      uint2 out[4];
      tr4x4_bf16(sta[t], out);
      const int q = r4 ^ (c4 & 14);
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        *(uint2*)(sA + (c4 * 4 + i) * LDK + q * 4) = out[i];
    }
    #pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int bid = t * 256 + tid;
      const int c4 = bid & (TN / 4 - 1);
      const int r4 = bid / (TN / 4);
      uint2 out[4];
      tr4x4_bf16(stb[t], out);
      const int q = r4 ^ (c4 & 14);
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        *(uint2*)(sB + (c4 * 4 + i) * LDK + q * 4) = out[i];
    }
  };
  auto mfma_all = [&]() {
    #pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      x8 af[4], bf[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int row = wm + mi * 16 + fr;
        const int q = ((ks + fk) >> 2) ^ ((row >> 2) & 14);
        af[mi] = *(const x8*)&sA[row * LDK + q * 4];
      }
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int row = wn + ni * 16 + fr;
        const int q = ((ks + fk) >> 2) ^ ((row >> 2) & 14);
        bf[ni] = *(const x8*)&sB[row * LDK + q * 4];
      }
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = Elem16<T>::mfma(af[mi], bf[ni], acc[mi][ni]);
    }
  };

  bool first = true;
  for (int kc = blockIdx.z; kc < nchunks; kc += gridDim.z) {
    const int kk0 = kc * BK;
    if (first) {
      issue_all(kk0);
      write_all();
      __syncthreads();
      first = false;
    }
    const int kn = kc + gridDim.z;
    const bool has_next = kn < nchunks;
    // chunk kn's global loads issue before chunk kc's MFMAs (latency cover)
    if (has_next) issue_all(kn * BK);
    mfma_all();
    if (has_next) {
      __syncthreads();
      write_all();
      __syncthreads();
    }
  }

  if constexpr (!DIRECT) {
    store_frag_slab<16>(dwp, &acc[0][0], tid);
    return;
  }
  const int dm = (lane >> 4) * 4;
  const int dn = lane & 15;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + ni * 16 + dn;
      if (n >= d.N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + dm + r;
        if (m >= d.M) continue;
        store_dw<T>(dwb, f32, (long)m * d.N + n, acc[mi][ni][r]);
      }
    }
}

// Sum the split-K partial slabs and emit the 16-bit channels_last weight grad:
// out[k][tap*Cout + c] (= memory layout of channels_last (K, Cout, R, S)).
// Cpad==Cout -> identity column map; the stem maps Cpad=4 -> Cout=3 and drops
// the zero-pad channel and any tap >= R*S.
template <typename T>
__global__ void wgrad_reduce_kernel(const float* __restrict__ part,
                                    void* __restrict__ dw, bool f32,
                                    long MN, int N, int Nout, int splits,
                                    int Cpad, int Cout) {
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < MN;
       o += (long)gridDim.x * blockDim.x) {
    const long m = o / N;
    const int n = (int)(o - m * N);
    int nout = n;
    if (Cpad != Cout) {
      const int tap = n / Cpad, c = n - tap * Cpad;
      if (c >= Cout || tap * Cout >= Nout) continue;
      nout = tap * Cout + c;
    }
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(long)z * MN + o];
    store_dw<T>(dw, f32, m * Nout + nout, s);
  }
}

// Reduce for fragment-order slabs (layout: see store_frag_slab). A "slot" is
// one f32x4 of one thread of one tile; slot e of every z slice sits at
// part[z * nslots + e], so the sum over z is a stride-nslots walk of 16-byte
// loads, coalesced across the threads of a slot group whatever the tile shape.
// A thread sums V floats of a slot (4: the whole slot, 16-byte loads; 1: a
// quarter, for small dw that must keep ZW == 1), and a block is ZW z-groups
// of 256/ZW consecutive units: small dw takes a larger ZW, or V == 1, so the
// grid still covers the chip.
// Summation order (fixed, so results are bit-reproducible for a given
// (wtile, splits)): z-group g adds z = g, g+ZW, g+2*ZW, ... in increasing
// order into one fp32 accumulator (loads double-buffered eight at a time,
// adds in sequence); then the group partials are added in the order g = 0,
// 1, .., ZW-1 through LDS. ZW == 1 is the plain z = 0, 1, 2, ... order of
// wgrad_reduce_kernel: the default path (splits == 0) uses it, so that its
// gradients keep the bits they always had.
// Un-permute: slot -> (tile, f, tid) -> rows m..m+3 and column n exactly as
// the MFMA accumulator maps them (NF fragments = NF/4 x 4 of 16x16 per wave,
// WGN waves along n); rows/columns past M/N (edge tiles) are dropped, and
// the stem's padded columns are mapped as in wgrad_reduce_kernel.
template <int V>
__device__ __forceinline__ f32x4 ld_frag(const float* p) {
  if constexpr (V == 4) return *(const f32x4*)p;
  else return f32x4{*p, 0.f, 0.f, 0.f};
}

template <typename T, int ZW, int V>
__global__ __launch_bounds__(256)
void wgrad_reduce_frag_kernel(const float* __restrict__ part,
                              void* __restrict__ dw, bool f32, int M, int N,
                              int tn,
                              long nslots, int splits, int NF, int WGN,
                              int Nout, int Cpad, int Cout) {
  static_assert(V == 4 || (V == 1 && ZW == 1), "V == 1 is sequential only");
  constexpr int SPB = 256 / ZW;  // units per block; nslots % 256 == 0
  constexpr int U = 8;           // loads per batch
  __shared__ f32x4 red[ZW > 1 ? 256 : 1];
  const int tid = threadIdx.x;
  const int zg = tid / SPB;
  const long u = (long)blockIdx.x * SPB + (tid % SPB);   // unit of V floats
  const float* p = part + u * V;
  const long zstride = nslots * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  f32x4 cur[U], nxt[U];
  // a slice past the end contributes +0.f, which leaves s as it is
  auto load = [&](f32x4 (&v)[U], int z0) {
    #pragma unroll
    for (int i = 0; i < U; ++i) {
      const int z = z0 + i * ZW;
      v[i] = z < splits ? ld_frag<V>(p + (long)z * zstride)
                        : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(cur, zg);
  for (int z0 = zg; z0 < splits; z0 += U * ZW) {
    const int zn = z0 + U * ZW;
    if (zn < splits) load(nxt, zn);   // in flight while cur is added
    #pragma unroll
    for (int i = 0; i < U; ++i) s += cur[i];
    if (zn < splits) {
      #pragma unroll
      for (int i = 0; i < U; ++i) cur[i] = nxt[i];
    }
  }
  if (ZW > 1) {
    red[tid] = s;
    __syncthreads();
    if (zg != 0) return;
    #pragma unroll
    for (int g = 1; g < ZW; ++g) s += red[g * SPB + tid];
  }
  const long e = u * V >> 2;               // slot
  const int r0 = (int)(u * V & 3);         // first of this thread's V rows
  const int per = NF * 256;
  const int tile = (int)(e / per);
  const int w = (int)(e - (long)tile * per);
  const int f = w >> 8, t = w & 255;
  const int wave = t >> 6, lane = t & 63;
  const int wtm = (NF >> 2) * 16;           // wave tile rows
  const int by = tile / tn, bx = tile - by * tn;
  const int m = by * (4 / WGN) * wtm + (wave / WGN) * wtm + (f >> 2) * 16 +
                (lane >> 4) * 4;
  const int n = bx * WGN * 64 + (wave % WGN) * 64 + (f & 3) * 16 + (lane & 15);
  if (n >= N) return;
  int nout = n;
  if (Cpad != Cout) {  // stem: drop the pad channel and taps >= R*S
    const int tap = n / Cpad, c = n - tap * Cpad;
    if (c >= Cout || tap * Cout >= Nout) return;
    nout = tap * Cout + c;
  }
  #pragma unroll
  for (int r = 0; r < V; ++r)
    if (m + r0 + r < M)
      store_dw<T>(dw, f32, (long)(m + r0 + r) * Nout + nout, s[r]);
}

// Reduce for the split-K fwd / dgrad slabs (conv_igemm_kernel<.., SPLITK>):
// out[m][n] = round(sum over z = 0, 1, .., S-1 of slab z), fp32 adds in that
// fixed order, one rounding to T, so a (shape, splits) pair always gives the
// same bits. A sibling of wgrad_reduce_frag_kernel<T, 1, 4>, not a reuse: that
// kernel gives a thread one slot (4 rows of ONE column), i.e. 2-byte stores
// 32 bytes apart across a wave. The output here is the activation-sized
// [M][N] tensor, so a thread takes the 8 consecutive slots of a lane octet
// instead — 4 rows x 8 consecutive channels, 128 contiguous bytes per slice
// to load and one 16-byte store per row — and threads are numbered so that 16
// consecutive threads cover one 256-byte row segment of the 128x128 tile.
// Thread q of a tile: column octet co = q & 15, row quad rq = q >> 4; the
// slot follows from the accumulator map of the 128x128 tile (wave order
// wm = (wave >> 1) * 64, wn = (wave & 1) * 64, f = mi * 4 + ni, row =
// (lane >> 4) * 4 + reg, col = lane & 15). Rows / columns past M / N (edge
// tiles) are dropped; N % 8 != 0 stores element by element.
// BNEPI: the evaluation epilogue of conv_igemm_kernel, applied to the summed
// value before the one rounding. The thread's 8 channels take two float4 of
// scale and of shift, and each row one 16-byte residual load at the address
// of the store it precedes; the N % 8 != 0 tail reads element by element.
template <typename T, bool BNEPI = false>
__global__ __launch_bounds__(256)
void igemm_reduce_frag_kernel(const float* __restrict__ part,
                              T* __restrict__ out, int M, int N, int tn,
                              long nslots, int splits,
                              typename EpiArg<T, BNEPI>::type ep) {
  typedef typename Elem16<T>::x8 x8;
  const long u = (long)blockIdx.x * 256 + threadIdx.x;  // grid = 2 * ntiles
  const int tile = (int)(u >> 9);
  const int q = (int)(u & 511);
  const int co = q & 15, rq = q >> 4;
  const int wave = ((rq >> 4) << 1) | (co >> 3);
  const int f = ((rq >> 2) & 3) * 4 + ((co >> 1) & 3);
  const int lane0 = (rq & 3) * 16 + (co & 1) * 8;
  const f32x4* p = (const f32x4*)part + (long)tile * 4096 + f * 256 +
                   wave * 64 + lane0;
  f32x4 s[8], cur[8], nxt[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    s[j] = p[j];
    cur[j] = nxt[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (splits > 1) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) cur[j] = p[nslots + j];
  }
  for (int z = 1; z < splits; ++z) {
    const bool more = z + 1 < splits;
    if (more) {   // slice z+1 in flight while slice z is added
      #pragma unroll
      for (int j = 0; j < 8; ++j) nxt[j] = p[(long)(z + 1) * nslots + j];
    }
    #pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += cur[j];
    if (more) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) cur[j] = nxt[j];
    }
  }
  const int by = tile / tn, bx = tile - by * tn;
  const int m = by * 128 + rq * 4;
  const int n = bx * 128 + co * 8;
  if (n >= N) return;
  const bool vec = (N & 7) == 0;   // then n + 8 <= N and rows are 16 B aligned
  if constexpr (BNEPI) {
    float sc[8], sh[8];
    if (vec) {
      *(float4*)&sc[0] = *(const float4*)(ep.scale + n);
      *(float4*)&sc[4] = *(const float4*)(ep.scale + n + 4);
      *(float4*)&sh[0] = *(const float4*)(ep.shift + n);
      *(float4*)&sh[4] = *(const float4*)(ep.shift + n + 4);
    } else {
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int nj = min(n + j, N - 1);
        sc[j] = ep.scale[nj];
        sh[j] = ep.shift[nj];
      }
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (m + r >= M) continue;
      const long o = (long)(m + r) * N + n;
      if (vec) {
        x8 rv = {}, v;
        if (ep.res != nullptr) rv = *(const x8*)(ep.res + o);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = fmaf(s[j][r], sc[j], sh[j]);
          if (ep.res != nullptr) f += (float)rv[j];
          if (ep.relu) f = fmaxf(f, 0.f);
          v[j] = Elem16<T>::from_float(f);
        }
        *(x8*)(out + o) = v;
      } else {
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (n + j >= N) continue;
          float f = fmaf(s[j][r], sc[j], sh[j]);
          if (ep.res != nullptr) f += (float)ep.res[o + j];
          if (ep.relu) f = fmaxf(f, 0.f);
          out[o + j] = Elem16<T>::from_float(f);
        }
      }
    }
    return;
  }
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (m + r >= M) continue;
    T* dst = out + (long)(m + r) * N + n;
    if (vec) {
      x8 v;
      #pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = Elem16<T>::from_float(s[j][r]);
      *(x8*)dst = v;
    } else {
      #pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n + j < N) dst[j] = Elem16<T>::from_float(s[j][r]);
    }
  }
}

// wT[c][i][j][k] = w[k][R-1-i][S-1-j][c] — the 180°-rotated transposed filter
// the dgrad GEMM consumes, built in ONE kernel (the ATen flip+permute+copy
// chain was 3 launches per conv backward). This kernel, the 16-bit source path
// of multi_build_wT_kernel and the two stem pad kernels below only copy
// 16-bit patterns (and write zero, all bits clear in either format): they are
// declared on __bf16 and take fp16 tensors through the same instantiation.
__global__ void build_wT_kernel(const __bf16* __restrict__ w,
                                __bf16* __restrict__ wT,
                                int K, int R, int S, int C) {
  const long total = (long)K * R * S * C;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (long)gridDim.x * blockDim.x) {
    const int k = (int)(o % K);
    long t = o / K;
    const int j = (int)(t % S); t /= S;
    const int i = (int)(t % R);
    const int c = (int)(t / R);
    wT[o] = w[(((long)k * R + (R - 1 - i)) * S + (S - 1 - j)) * C + c];
  }
}

// The same rotation for up to 32 filters in one launch, through an LDS tile
// transpose: a block takes one filter tap of one tensor, 64 k x 64 c. It
// reads 64 rows of 64 consecutive c (128 B of bf16 each) and writes 64 rows
// of 64 consecutive k (128 B each), where build_wT_kernel reads 2 bytes at
// stride R*S*C per lane. IT = float additionally rounds to OT (bf16 or fp16)
// and, where w16 is given, stores the rounded copy at the source index: cast
// + rotate of an fp32 weight in one pass (conv_prep_weight). A 16-bit IT is
// moved as it is, whichever format it holds. Rows move as 16-byte units
// when the row length is a multiple of 8 and the base is 16-byte aligned, and
// element by element otherwise (ragged C such as the 3-channel stem); either
// way consecutive lanes touch consecutive addresses, and K or C past the last
// full tile are predicated off.
constexpr int WT_MAX_TENSORS = 32;

struct WTList {
  const void* w[WT_MAX_TENSORS];   // [K][R*S][C], IT
  void* w16[WT_MAX_TENSORS];       // [K][R*S][C] 16-bit copy of w, or null
  void* wT[WT_MAX_TENSORS];        // [C][R*S][K], 16-bit
  int K[WT_MAX_TENSORS], C[WT_MAX_TENSORS], RS[WT_MAX_TENSORS];
  int nblocks[WT_MAX_TENSORS];     // RS * ceil(K/64) * ceil(C/64)
  int ntensors;
};

template <typename OT>
__device__ __forceinline__ unsigned short wt_bits(float v) {
  return __builtin_bit_cast(unsigned short, Elem16<OT>::from_float(v));
}
template <typename OT>
__device__ __forceinline__ unsigned short wt_bits(__bf16 v) {
  return __builtin_bit_cast(unsigned short, v);
}

template <typename IT, typename OT = __bf16>
__global__ __launch_bounds__(256)
void multi_build_wT_kernel(WTList tl) {
  // [k][c]; 33-dword rows keep the column reads of the store phase off the
  // same LDS bank
  __shared__ unsigned short tile[64][66];
  int b = blockIdx.x;
  int t = 0;
  for (; t < tl.ntensors; ++t) {
    if (b < tl.nblocks[t]) break;
    b -= tl.nblocks[t];
  }
  if (t >= tl.ntensors) return;
  const int K = tl.K[t], C = tl.C[t], RS = tl.RS[t];
  const int tc = (C + 63) / 64;
  const int c0 = (b % tc) * 64;
  const int tap = (b / tc) % RS;
  const int k0 = (b / tc / RS) * 64;
  const IT* __restrict__ w = (const IT*)tl.w[t];
  unsigned short* __restrict__ w16 = (unsigned short*)tl.w16[t];
  unsigned short* __restrict__ wT = (unsigned short*)tl.wT[t];
  const int tid = threadIdx.x;

  const bool vec_in = C % 8 == 0 && ((size_t)w & 15) == 0 &&
                      ((size_t)w16 & 15) == 0;
  if (vec_in) {
    const int lc = (tid & 7) * 8;
    #pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int kk = (tid >> 3) + 32 * ps;
      const int k = k0 + kk, c = c0 + lc;
      if (k >= K || c >= C) continue;
      const long idx = ((long)k * RS + tap) * C + c;
      uint4 v;
      if constexpr (sizeof(IT) == 4) {
        const float4 a = *(const float4*)(w + idx);
        const float4 bb = *(const float4*)(w + idx + 4);
        v.x = wt_bits<OT>(a.x) | ((unsigned)wt_bits<OT>(a.y) << 16);
        v.y = wt_bits<OT>(a.z) | ((unsigned)wt_bits<OT>(a.w) << 16);
        v.z = wt_bits<OT>(bb.x) | ((unsigned)wt_bits<OT>(bb.y) << 16);
        v.w = wt_bits<OT>(bb.z) | ((unsigned)wt_bits<OT>(bb.w) << 16);
        if (w16 != nullptr) *(uint4*)(w16 + idx) = v;
      } else {
        v = *(const uint4*)(w + idx);
      }
      unsigned* dst = (unsigned*)&tile[kk][lc];   // 4-byte aligned only
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
  } else {
    #pragma unroll 4
    for (int e = 0; e < 16; ++e) {
      const int i = tid + 256 * e;
      const int kk = i >> 6, cc = i & 63;
      const int k = k0 + kk, c = c0 + cc;
      if (k >= K || c >= C) continue;
      const long idx = ((long)k * RS + tap) * C + c;
      const unsigned short bits = wt_bits<OT>(w[idx]);
      if (sizeof(IT) == 4 && w16 != nullptr) w16[idx] = bits;
      tile[kk][cc] = bits;
    }
  }
  __syncthreads();

  const int tapT = RS - 1 - tap;   // (R-1-i, S-1-j) of tap (i, j)
  const bool vec_out = K % 8 == 0 && ((size_t)wT & 15) == 0;
  if (vec_out) {
    const int lk = (tid & 7) * 8;
    #pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int cc = (tid >> 3) + 32 * ps;
      const int k = k0 + lk, c = c0 + cc;
      if (k >= K || c >= C) continue;
      uint4 v;
      v.x = tile[lk + 0][cc] | ((unsigned)tile[lk + 1][cc] << 16);
      v.y = tile[lk + 2][cc] | ((unsigned)tile[lk + 3][cc] << 16);
      v.z = tile[lk + 4][cc] | ((unsigned)tile[lk + 5][cc] << 16);
      v.w = tile[lk + 6][cc] | ((unsigned)tile[lk + 7][cc] << 16);
      *(uint4*)(wT + ((long)c * RS + tapT) * K + k) = v;
    }
  } else {
    #pragma unroll 4
    for (int e = 0; e < 16; ++e) {
      const int i = tid + 256 * e;
      const int cc = i >> 6, kk = i & 63;
      const int k = k0 + kk, c = c0 + cc;
      if (k >= K || c >= C) continue;
      wT[((long)c * RS + tapT) * K + k] = tile[kk][cc];
    }
  }
}

// x4[p][0..3] = {x[p][0..2], 0} — NHWC C=3 -> C=4 (stem fast path). Two
// pixels per thread: 3 aligned dword loads -> 2 aligned dwordx2 stores.
__global__ void pad_c3_to_c4_kernel(const __bf16* __restrict__ x,
                                    __bf16* __restrict__ x4, long npix) {
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  const long pairs = (npix + 1) / 2;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < pairs;
       o += (long)gridDim.x * blockDim.x) {
    const long p = o * 2;
    __bf16 v[8] = {};
    if (p + 2 <= npix) {
      const float* src = (const float*)(x + p * 3);   // 12 B, 4 B aligned
      *(float*)&v[0] = src[0];
      *(float*)&v[2] = src[1];   // v[2],v[3] = {x[p][2], x[p+1][0]}
      *(float*)&v[6] = src[2];
      v[4] = v[3]; v[5] = v[6]; v[6] = v[7]; v[3] = (__bf16)0.f;
      v[7] = (__bf16)0.f;
    } else {  // odd tail pixel
      for (int c = 0; c < 3; ++c) v[c] = x[p * 3 + c];
    }
    float2* dst = (float2*)(x4 + p * 4);
    dst[0] = *(float2*)&v[0];
    if (p + 2 <= npix) dst[1] = *(float2*)&v[4];
  }
}

// w4[k][tap*4 + c] = w[k][tap*3 + c] for c<3, tap<R*S; else 0.
// Kpad = R*S*4 rounded up to BK. w is channels_last (K,3,R,S) = [K][R][S][3].
__global__ void pad_w_c4_kernel(const __bf16* __restrict__ w,
                                __bf16* __restrict__ w4,
                                int K, int RS, int Kpad) {
  const long total = (long)K * Kpad;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (long)gridDim.x * blockDim.x) {
    const int k = (int)(o / Kpad);
    const int n = (int)(o - (long)k * Kpad);
    const int tap = n >> 2, c = n & 3;
    w4[o] = (tap < RS && c < 3) ? w[((long)k * RS + tap) * 3 + c]
                                : (__bf16)0.f;
  }
}

hipStream_t conv_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline bool is_16bit(const at::Tensor& t) {
  return t.scalar_type() == at::ScalarType::BFloat16 ||
         t.scalar_type() == at::ScalarType::Half;
}

inline void check_nhwc_16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && is_16bit(t),
              name, " must be a bf16 or fp16 HIP tensor, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 4 &&
              (t.is_contiguous(at::MemoryFormat::ChannelsLast) ||
               t.is_contiguous()),
              name, " must be 4-D and dense");
}

// All 16-bit operands of one call share one format.
inline void check_same_16(const at::Tensor& a, const char* an,
                          const at::Tensor& b, const char* bn) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), an, " is ", a.scalar_type(),
              " but ", bn, " is ", b.scalar_type(),
              ": the 16-bit operands of a conv call must share one dtype");
}

// Pointer for the kernels that only move 16-bit patterns (either format).
inline const __bf16* bf16_ptr(const at::Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr());
}

template <typename T>
inline const T* ptr16(const at::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}

}  // namespace

at::Tensor conv_build_wT(at::Tensor w) {
  check_nhwc_16(w, "w");
  const int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  auto wT = at::empty({C, R, S, K}, w.options().memory_format(
                                        at::MemoryFormat::Contiguous));
  const long total = (long)K * R * S * C;
  const int blocks = (int)std::min((total + 255) / 256, (long)2048);
  hipLaunchKernelGGL(build_wT_kernel, dim3(blocks), dim3(256), 0,
                     conv_stream(), bf16_ptr(w),
                     reinterpret_cast<__bf16*>(wT.data_ptr()), K, R, S, C);
  return wT;
}

namespace {
// One WTList entry: src (K,C,R,S) channels_last -> wT (C,R,S,K) contiguous,
// with an optional 16-bit copy of an fp32 src. wT, w16 and a 16-bit src share
// one format.
int wt_fill(WTList& tl, int t, const at::Tensor& src, const at::Tensor* w16,
            const at::Tensor& wT) {
  TORCH_CHECK(src.is_cuda() && src.dim() == 4 &&
              src.is_contiguous(at::MemoryFormat::ChannelsLast),
              "build_wT: filter must be a 4-D channels_last HIP tensor");
  const long K = src.size(0), C = src.size(1), R = src.size(2), S = src.size(3);
  TORCH_CHECK(wT.is_cuda() && is_16bit(wT) &&
              wT.is_contiguous() && wT.dim() == 4 && wT.size(0) == C &&
              wT.size(1) == R && wT.size(2) == S && wT.size(3) == K,
              "build_wT: wT must be a contiguous bf16 or fp16 (C,R,S,K) tensor");
  if (w16 != nullptr) {
    TORCH_CHECK(w16->is_cuda() && is_16bit(*w16) &&
                w16->sizes() == src.sizes() &&
                w16->is_contiguous(at::MemoryFormat::ChannelsLast),
                "build_wT: w16 must be bf16 or fp16, channels_last, of the "
                "filter's shape");
    check_same_16(*w16, "w16", wT, "wT");
  } else {
    check_same_16(src, "the filter", wT, "wT");
  }
  const long nb = R * S * ((K + 63) / 64) * ((C + 63) / 64);
  TORCH_CHECK(K > 0 && C > 0 && R * S > 0 && nb < (1L << 24),
              "build_wT: filter too large");
  tl.w[t] = src.data_ptr();
  tl.w16[t] = w16 ? w16->data_ptr() : nullptr;
  tl.wT[t] = wT.data_ptr();
  tl.K[t] = (int)K; tl.C[t] = (int)C; tl.RS[t] = (int)(R * S);
  tl.nblocks[t] = (int)nb;
  return (int)nb;
}
}  // namespace

// wT[i] <- rotate(w16[i]) for every filter, one launch per 32 tensors.
void multi_tensor_build_wT(std::vector<at::Tensor> w16s,
                           std::vector<at::Tensor> wTs) {
  TORCH_CHECK(w16s.size() == wTs.size());
  auto stream = conv_stream();
  size_t i = 0;
  while (i < w16s.size()) {
    WTList tl;
    int nblocks = 0, t = 0;
    for (; t < WT_MAX_TENSORS && i < w16s.size(); ++t, ++i) {
      TORCH_CHECK(is_16bit(w16s[i]),
                  "multi_tensor_build_wT expects bf16 or fp16 filters");
      nblocks += wt_fill(tl, t, w16s[i], nullptr, wTs[i]);
    }
    tl.ntensors = t;
    hipLaunchKernelGGL(multi_build_wT_kernel<__bf16>, dim3(nblocks), dim3(256),
                       0, stream, tl);
  }
}

// w16 <- round(w32) to w16's format, wT <- rotate(w16), one launch.
void conv_prep_weight(at::Tensor w32, at::Tensor w16, at::Tensor wT) {
  TORCH_CHECK(w32.scalar_type() == at::kFloat,
              "conv_prep_weight expects an fp32 filter");
  WTList tl;
  const int nblocks = wt_fill(tl, 0, w32, &w16, wT);
  tl.ntensors = 1;
  auto* kern = w16.scalar_type() == at::kHalf
      ? multi_build_wT_kernel<float, _Float16>
      : multi_build_wT_kernel<float, __bf16>;
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), 0, conv_stream(), tl);
}

// tile: 0 = size heuristic, 64 or 128 = force that GEMM-M tile (the
// autotune cache in ops/conv.py measures both and pins the winner per shape).
namespace {
inline int pick_bmt(const ConvDims& d, long tile) {
  if (tile == 64 || tile == 128) return (int)tile;
  const long tiles128 = (long)((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN);
  return tiles128 < 384 ? 64 : 128;  // small-M: halve tile, double blocks
}

// Split-K for the 128x128 fwd / dgrad tile (tile == 228 with splits > 1; the
// caller has checked FAST and N >= 96). The request is clamped so that every
// slice has at least one BK tile and the slabs stay under ~96 MB; 1 means
// "launch the unsplit kernel".
inline int igemm_splits(const ConvDims& d, long splits) {
  const long tiles = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
  const long max_ws = std::max(1L, 96L * 1024 * 1024 / (tiles * 128 * 128 * 4));
  return (int)std::max(1L, std::min({splits, (long)(d.K / BK), max_ws}));
}

// One split-K launch + one reduce. The slabs are whole tiles in fragment
// order (see store_frag_slab), allocated from the caching allocator on the
// conv stream, so a hipGraph capture of the step still works.
template <typename T, int MODE, bool BNEPI = false>
void igemm_splitk_launch(const at::Tensor& a, const at::Tensor& b,
                         at::Tensor& out, const ConvDims& d, int splits,
                         typename EpiArg<T, BNEPI>::type ep = {}) {
  auto stream = conv_stream();
  const int tn = (d.N + 127) / 128, tm = (d.M + 127) / 128;
  const long nslots = (long)tm * tn * 4096;   // f32x4 per slice
  auto part = at::empty({(long)splits * nslots * 4},
                        a.options().dtype(at::kFloat));
  hipLaunchKernelGGL(
      (conv_igemm_kernel<T, MODE, true, 128, false, 128, true>),
      dim3(tn, tm, splits), dim3(256), 0, stream, ptr16<T>(a), ptr16<T>(b),
      reinterpret_cast<T*>(part.data_ptr()), d, NoEpi{});
  hipLaunchKernelGGL((igemm_reduce_frag_kernel<T, BNEPI>), dim3(2 * tm * tn),
                     dim3(256), 0, stream, part.data_ptr<float>(),
                     reinterpret_cast<T*>(out.data_ptr()), d.M, d.N, tn,
                     nslots, splits, ep);
}

// The three passes are written once over the element type T; the public
// wrappers below check the operands and pick T from their (shared) dtype.
// BNEPI: the same launches with the evaluation epilogue (conv_fwd_bn_igemm);
// `ep` then holds the checked coefficient and residual pointers.
template <typename T, bool BNEPI = false>
at::Tensor conv_fwd_igemm_t(at::Tensor x, at::Tensor w, long stride, long pad,
                            long tile, long splits,
                            typename EpiArg<T, BNEPI>::type ep = {},
                            const at::Tensor* residual = nullptr) {
  const int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C, "channel mismatch");
  const int P = (H + 2 * (int)pad - R) / (int)stride + 1;
  const int Q = (W + 2 * (int)pad - S) / (int)stride + 1;
  auto out = at::empty({Nb, K, P, Q},
                       x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto stream = conv_stream();
  if (residual != nullptr)
    TORCH_CHECK(residual->sizes() == out.sizes() &&
                residual->is_contiguous(at::MemoryFormat::ChannelsLast),
                "conv_fwd_bn_igemm: residual must be a channels_last tensor "
                "of the output's shape ", out.sizes(), ", got ",
                residual->sizes());

  if (C == 3) {
    // stem fast path: pad x and w to 4 channels, tap-wise dwordx2 gathers
    const int RS = R * S;
    const int Kpad = ((RS * 4 + BK - 1) / BK) * BK;
    const long npix = (long)Nb * H * W;
    auto x4 = at::empty({npix * 4}, x.options());
    auto w4 = at::empty({(long)K * Kpad}, w.options());
    {
      const int blocks = (int)std::min((npix / 2 + 255) / 256, (long)4096);
      hipLaunchKernelGGL(pad_c3_to_c4_kernel, dim3(std::max(blocks, 1)),
                         dim3(256), 0, stream, bf16_ptr(x),
                         reinterpret_cast<__bf16*>(x4.data_ptr()), npix);
      const long wtotal = (long)K * Kpad;
      hipLaunchKernelGGL(pad_w_c4_kernel,
                         dim3((int)std::min((wtotal + 255) / 256, (long)1024)),
                         dim3(256), 0, stream, bf16_ptr(w),
                         reinterpret_cast<__bf16*>(w4.data_ptr()), K, RS, Kpad);
    }
    ConvDims d{Nb, P, Q, H, W, 4, R, S, (int)stride, (int)pad,
               Nb * P * Q, K, Kpad};
    const int bmt = pick_bmt(d, tile);
    const dim3 grid((d.N + BN - 1) / BN, (d.M + bmt - 1) / bmt);
    auto* kern = bmt == 64
        ? conv_igemm_kernel<T, 0, false, 64, true, BN, false, BNEPI>
        : conv_igemm_kernel<T, 0, false, 128, true, BN, false, BNEPI>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream,
                       ptr16<T>(x4),
                       ptr16<T>(w4),
                       reinterpret_cast<T*>(out.data_ptr()), d, ep);
    return out;
  }

  ConvDims d{Nb, P, Q, H, W, C, R, S, (int)stride, (int)pad,
             Nb * P * Q, K, R * S * C};
  const bool fast = (C % BK == 0);
  if (tile == 228 && fast && d.N >= 96) {
    const int nz = igemm_splits(d, splits);
    if (nz > 1) {
      igemm_splitk_launch<T, 0, BNEPI>(x, w, out, d, nz, ep);
      return out;
    }
    // 128x128 tile: halves the N-tile count and with it the A re-reads
    const dim3 grid((d.N + 127) / 128, (d.M + 127) / 128);
    hipLaunchKernelGGL(
        (conv_igemm_kernel<T, 0, true, 128, false, 128, false, BNEPI>), grid,
        dim3(256), 0, stream, ptr16<T>(x), ptr16<T>(w),
        reinterpret_cast<T*>(out.data_ptr()), d, ep);
    return out;
  }
  const int bmt = pick_bmt(d, tile);
  const dim3 grid((d.N + BN - 1) / BN, (d.M + bmt - 1) / bmt);
  auto* kern = bmt == 64
      ? (fast ? conv_igemm_kernel<T, 0, true, 64, false, BN, false, BNEPI>
              : conv_igemm_kernel<T, 0, false, 64, false, BN, false, BNEPI>)
      : (fast ? conv_igemm_kernel<T, 0, true, BM, false, BN, false, BNEPI>
              : conv_igemm_kernel<T, 0, false, BM, false, BN, false, BNEPI>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream,
                     ptr16<T>(x), ptr16<T>(w),
                     reinterpret_cast<T*>(out.data_ptr()), d, ep);
  return out;
}

template <typename T>
at::Tensor conv_fwd_bn_igemm_t(const at::Tensor& x, const at::Tensor& w,
                               const at::Tensor& scale_shift,
                               const at::Tensor* residual, bool relu,
                               long stride, long pad, long tile, long splits) {
  const long K = w.size(0);
  BnEpi<T> ep;
  ep.scale = scale_shift.data_ptr<float>() + 2 * K;
  ep.shift = ep.scale + K;
  ep.res = residual != nullptr ? ptr16<T>(*residual) : nullptr;
  ep.relu = relu ? 1 : 0;
  return conv_fwd_igemm_t<T, true>(x, w, stride, pad, tile, splits, ep,
                                   residual);
}
}  // namespace

// conv_fwd_igemm with the evaluation-mode BatchNorm folded into the epilogue:
//   out = round(relu(conv(x, w) * scale[k] + shift[k] + residual))
// in one launch (tile 228 with splits > 1: the split-K launch and a reduce
// that applies it). scale_shift is the fp32 [4][K] table bn_fwd_apply reads:
// rows 2 and 3 are scale and shift. residual, if given, has the output's
// shape, dtype and channels_last layout. Inference only.
at::Tensor conv_fwd_bn_igemm(at::Tensor x, at::Tensor w,
                             at::Tensor scale_shift,
                             c10::optional<at::Tensor> residual, bool relu,
                             long stride, long pad, long tile, long splits) {
  check_nhwc_16(x, "x"); check_nhwc_16(w, "w");
  check_same_16(x, "x", w, "w");
  TORCH_CHECK(scale_shift.is_cuda() && scale_shift.is_contiguous() &&
              scale_shift.scalar_type() == at::kFloat &&
              scale_shift.dim() == 2 && scale_shift.size(0) == 4 &&
              scale_shift.size(1) == w.size(0),
              "conv_fwd_bn_igemm: scale_shift must be a contiguous fp32 [4][",
              w.size(0), "] HIP tensor (rows 2, 3 = scale, shift), got ",
              scale_shift.scalar_type(), " ", scale_shift.sizes());
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) {
    TORCH_CHECK(residual->is_cuda() && residual->dim() == 4,
                "conv_fwd_bn_igemm: residual must be a 4-D HIP tensor");
    check_same_16(x, "x", *residual, "residual");
  }
  // the split-K reduce reads its 8 channels as 16-byte vectors when K % 8 == 0
  if (w.size(0) % 8 == 0) {
    TORCH_CHECK((reinterpret_cast<uintptr_t>(scale_shift.data_ptr()) & 15) == 0
                && (!has_res || (reinterpret_cast<uintptr_t>(
                                     residual->data_ptr()) & 15) == 0),
                "conv_fwd_bn_igemm: scale_shift and residual must be 16-byte "
                "aligned");
  }
  const at::Tensor* res = has_res ? &*residual : nullptr;
  return x.scalar_type() == at::kHalf
      ? conv_fwd_bn_igemm_t<_Float16>(x, w, scale_shift, res, relu, stride,
                                      pad, tile, splits)
      : conv_fwd_bn_igemm_t<__bf16>(x, w, scale_shift, res, relu, stride, pad,
                                    tile, splits);
}

// out (N,K,P,Q) channels_last <- x (N,C,H,W) channels_last, w (K,C,R,S)
// channels_last (memory [K][R][S][C]); bf16 or fp16, out in the same dtype.
// splits > 1 together with tile 228: split-K over that many slices (clamped,
// see igemm_splits); every other tile, and a shape the 128x128 tile does not
// take, ignores it.
at::Tensor conv_fwd_igemm(at::Tensor x, at::Tensor w, long stride, long pad,
                          long tile, long splits) {
  check_nhwc_16(x, "x"); check_nhwc_16(w, "w");
  check_same_16(x, "x", w, "w");
  return x.scalar_type() == at::kHalf
      ? conv_fwd_igemm_t<_Float16>(x, w, stride, pad, tile, splits)
      : conv_fwd_igemm_t<__bf16>(x, w, stride, pad, tile, splits);
}

namespace {
template <typename T>
at::Tensor conv_dgrad_igemm_t(at::Tensor dy, at::Tensor wT, long H, long W,
                              long stride, long pad, long tile, long splits) {
  const int Nb = dy.size(0), K = dy.size(1), P = dy.size(2), Q = dy.size(3);
  const int C = wT.size(0), R = wT.size(1), S = wT.size(2);
  TORCH_CHECK(wT.size(3) == K, "channel mismatch");
  auto dx = at::empty({Nb, C, H, W},
                      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  ConvDims d{Nb, (int)H, (int)W, P, Q, K, R, S, (int)stride, (int)pad,
             Nb * (int)H * (int)W, C, R * S * K};
  const bool fast = (K % BK == 0);
  if (fast && stride == 2 && H % 2 == 0 && W % 2 == 0) {
    // parity-decomposed: one grid.z slice per (h%2, w%2) output class,
    // class-local M; wrong-parity taps are skipped inside the kernel.
    ConvDims d2 = d;
    d2.M = Nb * (int)(H / 2) * (int)(W / 2);
    // 1x1 s2: only class (0,0) receives anything — 3/4 of dx is zero.
    // memset + one class beats 4 classes computing mostly nothing.
    const int nclass = (R == 1 && S == 1 && pad == 0) ? 1 : 4;
    if (nclass == 1) {
      const hipError_t err = hipMemsetAsync(
          dx.data_ptr(), 0, dx.numel() * dx.element_size(), conv_stream());
      TORCH_CHECK(err == hipSuccess, "hipMemsetAsync failed: ",
                  hipGetErrorString(err));
    }
    const long t128 = (long)((d2.M + BM - 1) / BM) *
                      ((d2.N + BN - 1) / BN) * nclass;
    const int bmt = (tile == 64 || tile == 128) ? (int)tile
                                                : (t128 < 384 ? 64 : 128);
    const dim3 grid((d2.N + BN - 1) / BN, (d2.M + bmt - 1) / bmt, nclass);
    auto* kern = bmt == 64 ? conv_igemm_kernel<T, 2, true, 64>
                           : conv_igemm_kernel<T, 2, true, 128>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0,
                       conv_stream(), ptr16<T>(dy), ptr16<T>(wT),
                       reinterpret_cast<T*>(dx.data_ptr()), d2, NoEpi{});
    return dx;
  }
  if (tile == 228 && fast && d.N >= 96) {
    const int nz = igemm_splits(d, splits);
    if (nz > 1) {
      igemm_splitk_launch<T, 1>(dy, wT, dx, d, nz);
      return dx;
    }
    const dim3 grid((d.N + 127) / 128, (d.M + 127) / 128);
    hipLaunchKernelGGL((conv_igemm_kernel<T, 1, true, 128, false, 128>), grid,
                       dim3(256), 0, conv_stream(), ptr16<T>(dy), ptr16<T>(wT),
                       reinterpret_cast<T*>(dx.data_ptr()), d, NoEpi{});
    return dx;
  }
  const int bmt = pick_bmt(d, tile);
  const dim3 grid((d.N + BN - 1) / BN, (d.M + bmt - 1) / bmt);
  auto* kern = bmt == 64
      ? (fast ? conv_igemm_kernel<T, 1, true, 64>
              : conv_igemm_kernel<T, 1, false, 64>)
      : (fast ? conv_igemm_kernel<T, 1, true> : conv_igemm_kernel<T, 1, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, conv_stream(),
                     ptr16<T>(dy), ptr16<T>(wT),
                     reinterpret_cast<T*>(dx.data_ptr()), d, NoEpi{});
  return dx;
}
}  // namespace

// dx (N,C,H,W) channels_last <- dy (N,K,P,Q) channels_last,
// wT (C,R,S,K) CONTIGUOUS with taps 180°-rotated (built by the Python side);
// bf16 or fp16, dx in the same dtype. splits: as for conv_fwd_igemm; the
// stride-2 parity path ignores it.
at::Tensor conv_dgrad_igemm(at::Tensor dy, at::Tensor wT, long H, long W,
                            long stride, long pad, long tile, long splits) {
  check_nhwc_16(dy, "dy");
  TORCH_CHECK(wT.is_cuda() && is_16bit(wT) && wT.is_contiguous(),
              "wT must be a contiguous bf16 or fp16 HIP tensor");
  check_same_16(dy, "dy", wT, "wT");
  return dy.scalar_type() == at::kHalf
      ? conv_dgrad_igemm_t<_Float16>(dy, wT, H, W, stride, pad, tile, splits)
      : conv_dgrad_igemm_t<__bf16>(dy, wT, H, W, stride, pad, tile, splits);
}

// dw (K,C,R,S) channels_last <- dy, x; in their 16-bit dtype, or with out_fp32
// the same 16-bit-rounded values as fp32 (the gradient of an fp32 parameter,
// with no cast kernel between the epilogue and the optimizer). Two-stage
// split-K: private fp32
// partial slabs per grid.z slice (fragment order, see store_frag_slab) + one
// reduce pass (no atomics); splits==1 non-stem collapses to a DIRECT 16-bit
// store. `splits`: 0 = default (~1024 blocks, plain z order: the bits this
// path has always produced), < 0 = one resident set of blocks, > 0 = as given.
// `wtile`: 0 = shape heuristic, 1 = v1 64x128, 2 = v2 128x128, 3 = v2 256x64
// (the autotune cache measures and pins these per shape).
namespace {
// Blocks per CU the split heuristic aims at, per tile family (resolved wtile).
// v2 / LIN are __launch_bounds__(256, 2): two blocks are resident per CU, and
// the split sweep has its optimum there (1x: +40-70 %; 3x, a partial second
// round: +15-35 %; 4x: up to +11 %). v1 (27 KB LDS, ~60 VGPRs) fits five;
// its sweep is flat from 3x to 5x with the minimum at 4x
// (profiles/r4_wgrad_split_sweep.txt).
inline int wgrad_blocks_per_cu(int tile) {
  return (tile == 1 || tile == 4) ? 4 : 2;
}

template <typename T>
at::Tensor conv_wgrad_igemm_t(at::Tensor dy, at::Tensor x, long R, long S,
                              long stride, long pad, long splits_arg,
                              long wtile, bool out_fp32) {
  const int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = dy.size(1), P = dy.size(2), Q = dy.size(3);
  auto stream = conv_stream();
  // out_fp32: same shape and strides, the 16-bit-rounded values widened
  auto dw = at::empty({K, C, R, S},
                      x.options().memory_format(at::MemoryFormat::ChannelsLast)
                          .dtype(out_fp32 ? at::kFloat : x.scalar_type()));

  const bool stem = (C == 3);
  int Cpad = C, Npad = (int)(R * S * C);
  at::Tensor x4;
  const T* xp = ptr16<T>(x);
  if (stem) {
    const long npix = (long)Nb * H * W;
    x4 = at::empty({npix * 4}, x.options());
    const int blocks = (int)std::min((npix / 2 + 255) / 256, (long)4096);
    hipLaunchKernelGGL(pad_c3_to_c4_kernel, dim3(std::max(blocks, 1)),
                       dim3(256), 0, stream, bf16_ptr(x),
                       reinterpret_cast<__bf16*>(x4.data_ptr()), npix);
    xp = ptr16<T>(x4);
    Cpad = 4;
    Npad = (int)(R * S * 4);
  }

  ConvDims d{Nb, P, Q, H, W, Cpad, (int)R, (int)S, (int)stride, (int)pad,
             K, Npad, Nb * P * Q};
  const bool fast = (C % BK == 0) && (K % 16 == 0);

  // tile pick: v2's larger tiles read dy/x fewer times (traffic per pass
  // scales with the tile count along the other axis) and stage with wide
  // LDS writes; LIN (1x1 s1 p0: both operands plain row-major) adds the
  // register-pipelined double buffer; v1 remains for small-M shapes and
  // the generic/stem paths
  const bool lin_ok = fast && !stem && R == 1 && S == 1 &&
                      stride == 1 && pad == 0;
  int tile = (int)wtile;
  if (tile == 0) {
    if (lin_ok && d.M >= 128 && d.N >= 96) tile = 5;
    else if (lin_ok && d.M >= 256 && d.N <= 64) tile = 6;
    else if (fast && !stem && d.M >= 256 && d.N <= 64) tile = 3;
    else if (fast && !stem && d.M >= 128 && d.N >= 96) tile = 2;
    else tile = 1;
  }
  if ((tile == 5 || tile == 6) && !lin_ok) tile = tile - 3;  // 2 / 3
  if (!fast || stem) tile = (tile == 4) ? 4 : 1;  // v2 needs the FAST layout
  const int TM = (tile == 3 || tile == 6 || tile == 9) ? 256
               : (tile == 2 || tile == 5 || tile == 8) ? 128 : 64;
  const int TN = (tile == 2 || tile == 5 || tile == 8) ? 128
               : (tile == 3 || tile == 6 || tile == 9) ? 64 : 128;

  const int tm = (d.M + TM - 1) / TM, tn = (d.N + TN - 1) / TN;
  const int nchunks = (d.K + BK - 1) / BK;
  // wide-stage v2 (wtile 8/9) strides 128-row stages: a z-slice beyond the
  // stage count would leave its partial slab unwritten
  const int nzmax = (tile == 8 || tile == 9) ? (nchunks + 1) / 2 : nchunks;
  // splits < 0, residency-sized: one resident set of blocks (CUs x blocks
  // per CU, see wgrad_blocks_per_cu) — every slice beyond that queues behind
  // the first round and only adds a TM*TN fp32 slab to write and re-read.
  // splits == 0, the default: the ~1024 blocks this path has always used,
  // summed in plain z order. Slice count and order decide the last bit of a
  // bf16 gradient, and a training run amplifies that bit (25 flagship steps
  // turn it into 18 % of the parameter norm), so the default keeps both and
  // with them every bit of a --reproducible run; the autotuner measures the
  // residency-sized count as one of its candidates. Either way keep >=8
  // chunks per block (fewer and the per-block fill/drain + slab traffic
  // dominates — measured on the CIFAR shapes, where over-splitting cost 2-4x)
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int target = splits_arg < 0 ? cus * wgrad_blocks_per_cu(tile) : 1024;
  int splits = (splits_arg > 0) ? (int)splits_arg
                                : std::min(target / (tm * tn), nchunks / 8);
  // bound the partial-slab workspace to ~96 MB (slabs hold whole tiles)
  const long max_ws = 96L * 1024 * 1024 / ((long)tm * tn * TM * TN * 4);
  splits = std::max(1, (int)std::min({(long)splits, (long)nzmax,
                                      std::max(max_ws, 1L), 1024L}));
  const dim3 grid(tn, tm, splits);

  if (splits == 1 && !stem && tile != 4) {
    auto* kern =
        tile == 9 ? conv_wgrad_v2_kernel<T, 4, 1, true, 2>
        : tile == 8 ? conv_wgrad_v2_kernel<T, 2, 2, true, 2>
        : tile == 6 ? conv_wgrad_lin_kernel<T, 4, 1, true>
        : tile == 5 ? conv_wgrad_lin_kernel<T, 2, 2, true>
        : tile == 3 ? conv_wgrad_v2_kernel<T, 4, 1, true>
        : tile == 2 ? conv_wgrad_v2_kernel<T, 2, 2, true>
        : (fast ? conv_wgrad_kernel<T, true, false, true>
                : conv_wgrad_kernel<T, false, false, true>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, ptr16<T>(dy), xp,
                       nullptr, dw.data_ptr(), d, out_fp32);
    return dw;
  }

  const bool atomic = (tile == 4);
  const bool rowmajor = atomic;           // else fragment-order slabs
  const long MN = (long)d.M * d.N;
  const long slab = rowmajor ? MN : (long)tm * tn * TM * TN;
  auto part = atomic
      ? at::zeros({MN}, x.options().dtype(at::kFloat))
      : at::empty({(long)splits * slab}, x.options().dtype(at::kFloat));
  auto* kern =
      tile == 9 ? conv_wgrad_v2_kernel<T, 4, 1, false, 2>
      : tile == 8 ? conv_wgrad_v2_kernel<T, 2, 2, false, 2>
      : tile == 6 ? conv_wgrad_lin_kernel<T, 4, 1, false>
      : tile == 5 ? conv_wgrad_lin_kernel<T, 2, 2, false>
      : tile == 3 ? conv_wgrad_v2_kernel<T, 4, 1, false>
      : tile == 2 ? conv_wgrad_v2_kernel<T, 2, 2, false>
      : atomic ? (stem ? conv_wgrad_kernel<T, false, true, false, true>
                 : fast ? conv_wgrad_kernel<T, true, false, false, true>
                        : conv_wgrad_kernel<T, false, false, false, true>)
      : stem ? conv_wgrad_kernel<T, false, true, false>
             : (fast ? conv_wgrad_kernel<T, true, false, false>
                     : conv_wgrad_kernel<T, false, false, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, ptr16<T>(dy), xp,
                     part.data_ptr<float>(), nullptr, d, out_fp32);
  if (!rowmajor) {
    const int NF = TM * TN / 1024;         // f32x4 fragments per thread
    const long nslots = slab / 4;
    // smallest z-group count that gives the reduce two blocks per CU, while
    // every group still has four slices to keep in flight; the default path
    // keeps plain z order and narrows the per-thread unit instead
    const bool seq = (splits_arg == 0);
    int zw = 1;
    while (!seq && zw < 16 && nslots * zw / 256 < 2L * cus && zw * 8 <= splits)
      zw *= 2;
    const int v = (seq && nslots / 256 < 2L * cus) ? 1 : 4;
    auto* red = v == 1 ? wgrad_reduce_frag_kernel<T, 1, 1>
              : zw == 1 ? wgrad_reduce_frag_kernel<T, 1, 4>
              : zw == 2 ? wgrad_reduce_frag_kernel<T, 2, 4>
              : zw == 4 ? wgrad_reduce_frag_kernel<T, 4, 4>
              : zw == 8 ? wgrad_reduce_frag_kernel<T, 8, 4>
                        : wgrad_reduce_frag_kernel<T, 16, 4>;
    hipLaunchKernelGGL(red, dim3((unsigned)(nslots * zw * (4 / v) / 256)),
                       dim3(256), 0, stream, part.data_ptr<float>(),
                       dw.data_ptr(), out_fp32, d.M, d.N, tn, nslots, splits,
                       NF, TN / 64, (int)(R * S * C), Cpad, C);
    return dw;
  }
  hipLaunchKernelGGL(wgrad_reduce_kernel<T>,
                     dim3((int)std::min((MN + 255) / 256, (long)4096)),
                     dim3(256), 0, stream, part.data_ptr<float>(),
                     dw.data_ptr(), out_fp32, MN, d.N,
                     (int)(R * S * C), atomic ? 1 : splits, Cpad, C);
  return dw;
}
}  // namespace

at::Tensor conv_wgrad_igemm(at::Tensor dy, at::Tensor x, long R, long S,
                            long stride, long pad, long splits_arg,
                            long wtile, bool out_fp32) {
  check_nhwc_16(dy, "dy"); check_nhwc_16(x, "x");
  check_same_16(dy, "dy", x, "x");
  return x.scalar_type() == at::kHalf
      ? conv_wgrad_igemm_t<_Float16>(dy, x, R, S, stride, pad, splits_arg,
                                     wtile, out_fp32)
      : conv_wgrad_igemm_t<__bf16>(dy, x, R, S, stride, pad, splits_arg,
                                   wtile, out_fp32);
}
