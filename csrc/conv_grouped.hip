// MI355X (gfx950/CDNA4) grouped 3x3 convolution — NHWC bf16 or fp16, fp32
// accumulation, pad 1, stride 1 or 2, in_channels == out_channels == C,
// channels per group Cg in {4, 8, 16, 32, 64}.
//
// Packs. Channels are processed in packs of P = max(Cg, 32) consecutive
// channels: 32 / Cg whole groups, or one group at Cg 32 / 64. Inside a pack
// the convolution is dense P -> P with a block-diagonal filter (the
// off-diagonal Cg x Cg blocks are zero, written out by grouped_prep_kernel),
// so every MFMA is a full v_mfma_f32_16x16x32 with one filter tap as its K
// step (two steps at P = 64) and the addressing is the same for every group
// width. The redundant arithmetic (8x at Cg = 4) is spent on a layer whose
// useful intensity is far under the MFMA roof.
//
// fwd / dgrad (conv_grouped_kernel): direct convolution from an LDS patch. A
// block of 256 threads owns one pack, one image and one TH x 16 tile of
// output pixels. It stages the (TH*s+2) x (16*s+2) halo patch of its P
// channels (zeros outside the image) and the pack's 9 x P x P filter into
// LDS once; the nine taps then read shifted windows of the patch. The filter
// is the MFMA A operand and the pixels the B operand, so a lane's four
// accumulator rows are four consecutive output channels of one pixel: the
// epilogue rounds once and stores 8 bytes per lane. The input gradient is
// the same kernel on dy with the rotated operand; at stride 2 dy is staged
// zero-inserted (ZINS) and the stride-1 tap loop runs over it.
//
// wgrad (conv_grouped_wgrad_kernel + grouped_wgrad_reduce_kernel): per pack
// and tap a P x P GEMM reduced over all output pixels. Both MFMA operands
// need pixels along K, so dy and x are transposed in registers while they
// are staged (8 pixels x 8 channels per thread) and kept channel-major in
// LDS; x is kept in three copies, one per filter column j, each holding only
// the columns ow*s + j - 1, which makes every fragment read one aligned
// ds_read_b128 for either stride. Blocks own a pack and a contiguous range
// of tiles and dump fp32 partial slabs; the reduce sums the splits in fixed
// order, keeps the diagonal blocks and rounds once. No atomics, no memset.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <tuple>

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are switched off for the
// device code of this file. Nothing here wants them: the fp32 work is MFMA
// accumulation, one rounding per output and the scalar sum of the reduce, and
// the compiler emits none with the feature on either, so this costs nothing;
// it keeps that true if the fp32 code grows.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                                 \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// Local copy of conv_igemm.hip's Elem16 (that one lives in its file's
// anonymous namespace), plus the 4-wide vector of the 8-byte epilogue store.
template <typename T> struct Elem16;

template <> struct Elem16<__bf16> {
  typedef __attribute__((ext_vector_type(8))) __bf16 x8;
  typedef __attribute__((ext_vector_type(4))) __bf16 x4;
  static __device__ __forceinline__ f32x4 mfma(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ __bf16 from_float(float v) {
    return (__bf16)v;
  }
};

template <> struct Elem16<_Float16> {
  typedef __attribute__((ext_vector_type(8))) _Float16 x8;
  typedef __attribute__((ext_vector_type(4))) _Float16 x4;
  static __device__ __forceinline__ f32x4 mfma(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ _Float16 from_float(float v) {
    return (_Float16)v;
  }
};

constexpr int TW = 16;    // tile width in output pixels: one MFMA N fragment
constexpr int WTH = 8;    // wgrad tile height
constexpr int PADE = 8;   // LDS row padding in elements (16 bytes)

struct GDims {
  int Nb, C;
  int SH, SW;    // extents of the tensor that is read (x; dy for dgrad)
  int VH, VW;    // extents the taps index: SH, SW, or dx's under ZINS
  int OH, OW;    // extents of the tensor that is written
  int tiles_h, tiles_w;
};

// ---------------------------------------------------------------------------
// Weight prep: (C, Cg, 3, 3) -> wf, wb [C/P][9][P][P] with the zeros written.
//   wf[pack][i*3+j][k][c] = w[pack*P + k][c % Cg][i][j]      (fwd: A rows = k)
//   wb[pack][i*3+j][c][k] = w[pack*P + k][c % Cg][2-i][2-j]  (dgrad: A rows = c)
// for k, c of one group, else 0. The filter is read through its strides.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void grouped_prep_kernel(const unsigned short* __restrict__ w,
                         unsigned short* __restrict__ wf,
                         unsigned short* __restrict__ wb, long total, int Cg,
                         int P, long sk, long sc, long sr, long ss) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (long)gridDim.x * 256) {
    const int col = (int)(idx % P);
    const int row = (int)((idx / P) % P);
    const int tap = (int)((idx / ((long)P * P)) % 9);
    const long pack = idx / (9L * P * P);
    const int i = tap / 3, j = tap % 3;
    unsigned short f = 0, b = 0;
    if (row / Cg == col / Cg) {
      f = w[(pack * P + row) * sk + (col % Cg) * sc + i * sr + j * ss];
      b = w[(pack * P + col) * sk + (row % Cg) * sc + (2 - i) * sr +
            (2 - j) * ss];
    }
    wf[idx] = f;
    wb[idx] = b;
  }
}

// ---------------------------------------------------------------------------
// fwd / dgrad
// ---------------------------------------------------------------------------
// S = the stride the taps walk the patch with; ZINS = the source is staged
// zero-inserted (stride-2 input-grad: patch position (u, v) of the virtual
// VH x VW image holds src[u/2][v/2] when both are even, else 0), S is 1 then.
// TH = tile height, a multiple of 4: every wave owns TH/4 output rows and all
// P/16 channel fragments of them.
template <typename T, int P, int S, int TH, bool ZINS>
__global__ __launch_bounds__(256)
void conv_grouped_kernel(const T* __restrict__ src, const T* __restrict__ wp,
                         T* __restrict__ out, GDims d) {
  typedef typename Elem16<T>::x8 x8;
  typedef typename Elem16<T>::x4 x4;
  static_assert(!ZINS || S == 1, "the zero-inserted patch is walked at 1");
  constexpr int LDP = P + PADE;   // pixel stride of the patch, row stride of
                                  // the filter: 80 / 144 bytes, so 16 lanes'
                                  // 16-byte reads spread over the banks
  constexpr int PH = TH * S + 2, PW = TW * S + 2;
  constexpr int CH = P / 8;       // 16-byte chunks per pixel / filter row
  constexpr int MF = P / 16, KS = P / 32, RPW = TH / 4;
  __shared__ __attribute__((aligned(16))) T patch[PH * PW * LDP];
  __shared__ __attribute__((aligned(16))) T filt[9 * P * LDP];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pack = blockIdx.y, n = blockIdx.z;
  const int oh0 = (blockIdx.x / d.tiles_w) * TH;
  const int ow0 = (blockIdx.x % d.tiles_w) * TW;
  const int gu0 = oh0 * S - 1, gv0 = ow0 * S - 1;

  const T* wsrc = wp + (size_t)pack * 9 * P * P;
  for (int idx = tid; idx < 9 * P * CH; idx += 256) {
    const int row = idx / CH, ch = idx % CH;
    *reinterpret_cast<u32x4*>(filt + row * LDP + ch * 8) =
        *reinterpret_cast<const u32x4*>(wsrc + row * P + ch * 8);
  }
  const T* sbase = src + (size_t)n * d.SH * d.SW * d.C + (size_t)pack * P;
  for (int idx = tid; idx < PH * PW * CH; idx += 256) {
    const int pix = idx / CH, ch = idx % CH;
    const int gu = gu0 + pix / PW, gv = gv0 + pix % PW;
    bool ok = gu >= 0 && gu < d.VH && gv >= 0 && gv < d.VW;
    int sy = gu, sx = gv;
    if (ZINS) {
      ok = ok && ((gu | gv) & 1) == 0;
      sy = gu >> 1;
      sx = gv >> 1;
    }
    ok = ok && sy < d.SH && sx < d.SW;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok)
      v = *reinterpret_cast<const u32x4*>(
          sbase + ((size_t)sy * d.SW + sx) * d.C + ch * 8);
    *reinterpret_cast<u32x4*>(patch + pix * LDP + ch * 8) = v;
  }
  __syncthreads();

  const int l16 = lane & 15, kg = lane >> 4;
  f32x4 acc[RPW][MF];
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) acc[rr][mf] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int i = tap / 3, j = tap % 3;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      x8 a[MF];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        a[mf] = *reinterpret_cast<const x8*>(
            filt + (tap * P + mf * 16 + l16) * LDP + ks * 32 + kg * 8);
#pragma unroll
      for (int rr = 0; rr < RPW; ++rr) {
        const int pr = wave * RPW + rr;
        const x8 b = *reinterpret_cast<const x8*>(
            patch + ((pr * S + i) * PW + l16 * S + j) * LDP + ks * 32 +
            kg * 8);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf)
          acc[rr][mf] = Elem16<T>::mfma(a[mf], b, acc[rr][mf]);
      }
    }
  }

  // lane: pixel column l16, channels mf*16 + kg*4 .. +3 of its rows
  const int ow = ow0 + l16;
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int oh = oh0 + wave * RPW + rr;
    if (oh < d.OH && ow < d.OW) {
      T* o = out + (((size_t)n * d.OH + oh) * d.OW + ow) * d.C +
             (size_t)pack * P + kg * 4;
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          r[e] = Elem16<T>::from_float(acc[rr][mf][e]);
        *reinterpret_cast<x4*>(o + mf * 16) = r;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------
// Eight pixels x eight channels, one 16-byte load per pixel, come out as
// eight 16-byte rows of one channel each.
__device__ __forceinline__ void transpose8x8(const u32x4 (&in)[8],
                                             u16x8 (&outv)[8]) {
  u16x8 v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = __builtin_bit_cast(u16x8, in[e]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) outv[c][e] = v[e][c];
}

// GDims here: SH, SW = x's extents, OH, OW = dy's. Block (split, pack) runs
// the tiles [T*split/splits, T*(split+1)/splits) of the T = Nb*tiles_h*tiles_w
// tiles and writes slab[split][pack][tap][c][k] (k fastest: a lane's four
// accumulator rows are one 16-byte store).
template <typename T, int P, int S>
__global__ __launch_bounds__(256)
void conv_grouped_wgrad_kernel(const T* __restrict__ dy,
                               const T* __restrict__ x,
                               float* __restrict__ slab, GDims d) {
  typedef typename Elem16<T>::x8 x8;
  constexpr int PH = WTH * S + 2;
  constexpr int NPX = WTH * TW;          // 128 output pixels: 4 K steps
  constexpr int LDY = NPX + PADE;        // dyT[k][pixel]
  constexpr int LDX = PH * TW + PADE;    // xT[j][c][patch row][16 columns]
  constexpr int CH = P / 8;
  constexpr int NFR = P / 16;
  constexpr int NFW = NFR * NFR / 4;     // fragments per wave and tap: 1 | 4
  __shared__ __attribute__((aligned(16))) T dyT[P * LDY];
  __shared__ __attribute__((aligned(16))) T xT[3 * P * LDX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pack = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
  const int l16 = lane & 15, kg = lane >> 4;
  const int mf = (wave * NFW) / NFR, nf0 = (wave * NFW) % NFR;
  const long total = (long)d.Nb * d.tiles_h * d.tiles_w;
  const int t0 = (int)(total * split / splits);
  const int t1 = (int)(total * (split + 1) / splits);

  f32x4 acc[9][NFW];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int nf = 0; nf < NFW; ++nf) acc[tap][nf] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = t0; t < t1; ++t) {
    const int tw = t % d.tiles_w;
    const int th = (t / d.tiles_w) % d.tiles_h;
    const int n = t / (d.tiles_w * d.tiles_h);
    const int oh0 = th * WTH, ow0 = tw * TW;
    if (t != t0) __syncthreads();   // the last tile's reads are done

    // dy tile -> dyT: units of (row, half row, 8-channel chunk)
    const T* dbase = dy + (size_t)n * d.OH * d.OW * d.C + (size_t)pack * P;
    for (int u = tid; u < WTH * 2 * CH; u += 256) {
      const int ch = u % CH, half = (u / CH) & 1, pr = u / (2 * CH);
      const int oh = oh0 + pr;
      u32x4 in[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ow = ow0 + half * 8 + e;
        in[e] = u32x4{0u, 0u, 0u, 0u};
        if (oh < d.OH && ow < d.OW)
          in[e] = *reinterpret_cast<const u32x4*>(
              dbase + ((size_t)oh * d.OW + ow) * d.C + ch * 8);
      }
      u16x8 tr[8];
      transpose8x8(in, tr);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        *reinterpret_cast<u16x8*>(dyT + (ch * 8 + c) * LDY + pr * TW +
                                  half * 8) = tr[c];
    }
    // x patch -> xT: units of (column shift j, patch row, half row, chunk);
    // copy j holds the input columns (ow0 + pc) * S + j - 1, pc = 0..15
    const T* xbase = x + (size_t)n * d.SH * d.SW * d.C + (size_t)pack * P;
    for (int u = tid; u < 3 * PH * 2 * CH; u += 256) {
      const int ch = u % CH, half = (u / CH) & 1;
      const int pu = (u / (2 * CH)) % PH, j = u / (2 * CH * PH);
      const int gu = oh0 * S - 1 + pu;
      u32x4 in[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int gv = (ow0 + half * 8 + e) * S + j - 1;
        in[e] = u32x4{0u, 0u, 0u, 0u};
        if (gu >= 0 && gu < d.SH && gv >= 0 && gv < d.SW)
          in[e] = *reinterpret_cast<const u32x4*>(
              xbase + ((size_t)gu * d.SW + gv) * d.C + ch * 8);
      }
      u16x8 tr[8];
      transpose8x8(in, tr);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        *reinterpret_cast<u16x8*>(xT + (j * P + ch * 8 + c) * LDX + pu * TW +
                                  half * 8) = tr[c];
    }
    __syncthreads();

    // K index kg*8 + e of step ks is the tile pixel ks*32 + kg*8 + e: row
    // ks*2 + kg/2, columns (kg&1)*8 + e, for both operands
#pragma unroll
    for (int ks = 0; ks < NPX / 32; ++ks) {
      const int pr = ks * 2 + (kg >> 1), pc0 = (kg & 1) * 8;
      const x8 a = *reinterpret_cast<const x8*>(
          dyT + (mf * 16 + l16) * LDY + pr * TW + pc0);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int i = tap / 3, j = tap % 3;
#pragma unroll
        for (int nf = 0; nf < NFW; ++nf) {
          const x8 b = *reinterpret_cast<const x8*>(
              xT + (j * P + (nf0 + nf) * 16 + l16) * LDX +
              (pr * S + i) * TW + pc0);
          acc[tap][nf] = Elem16<T>::mfma(a, b, acc[tap][nf]);
        }
      }
    }
  }

  // lane: c = nf*16 + l16, k = mf*16 + kg*4 .. +3
  float* sb = slab + ((size_t)split * gridDim.x + pack) * 9 * P * P;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int nf = 0; nf < NFW; ++nf)
      *reinterpret_cast<f32x4*>(sb + ((size_t)tap * P + (nf0 + nf) * 16 +
                                      l16) * P + mf * 16 + kg * 4) =
          acc[tap][nf];
}

// dw (C, Cg, 3, 3) channels_last: offset k*9*Cg + tap*Cg + cg. Sums the
// splits in increasing order, so the result depends on (shape, splits) only.
template <typename T>
__global__ __launch_bounds__(256)
void grouped_wgrad_reduce_kernel(const float* __restrict__ slab,
                                 T* __restrict__ dw, long total, int Cg, int P,
                                 int splits, long split_stride) {
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total;
       o += (long)gridDim.x * 256) {
    const int cg = (int)(o % Cg);
    const int tap = (int)((o / Cg) % 9);
    const long k = o / (9L * Cg);
    const long pack = k / P;
    const int kl = (int)(k % P);
    const int cl = (kl / Cg) * Cg + cg;
    const float* p = slab + ((pack * 9 + tap) * P + cl) * P + kl;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += p[(long)z * split_stride];
    dw[o] = Elem16<T>::from_float(s);
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
hipStream_t grouped_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

inline bool is_16bit(const at::Tensor& t) {
  return t.scalar_type() == at::ScalarType::BFloat16 ||
         t.scalar_type() == at::ScalarType::Half;
}

inline void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && is_16bit(t), name,
              " must be a bf16 or fp16 HIP tensor, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, " must be 4-D channels_last");
  TORCH_CHECK(t.numel() > 0 && t.size(0) <= 65535, name,
              ": batch must be in 1..65535");
}

inline void check_same_16(const at::Tensor& a, const char* an,
                          const at::Tensor& b, const char* bn) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), an, " is ", a.scalar_type(),
              " but ", bn, " is ", b.scalar_type(),
              ": the 16-bit operands of a conv call must share one dtype");
}

inline int pack_width(long C, long groups) {
  TORCH_CHECK(groups >= 1 && C % groups == 0, "C must be a multiple of groups");
  const long Cg = C / groups;
  TORCH_CHECK(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64,
              "grouped conv: channels per group must be 4, 8, 16, 32 or 64, "
              "got ", Cg);
  const int P = Cg > 32 ? (int)Cg : 32;
  TORCH_CHECK(C % P == 0, "grouped conv: C must be a multiple of ", P);
  return P;
}

// The packed operand [C/P][9][P][P] of a C-channel tensor; returns P.
inline int check_packed(const at::Tensor& wp, long C, const at::Tensor& act) {
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.size(1) == 9 && wp.size(2) == wp.size(3) &&
              (wp.size(2) == 32 || wp.size(2) == 64) &&
              wp.size(0) * wp.size(2) == C,
              "grouped conv: the packed filter must be a contiguous "
              "[C/P][9][P][P] tensor from conv_grouped_prep");
  check_same_16(act, "the activation", wp, "the packed filter");
  return (int)wp.size(2);
}

inline long out_extent(long in, long stride) { return (in - 1) / stride + 1; }

template <typename T, int P, int S, int TH, bool ZINS>
void launch_grouped_t(const at::Tensor& src, const at::Tensor& wp,
                      at::Tensor& out, GDims d) {
  d.tiles_h = (d.OH + TH - 1) / TH;
  d.tiles_w = (d.OW + TW - 1) / TW;
  const dim3 grid(d.tiles_h * d.tiles_w, d.C / P, d.Nb);
  hipLaunchKernelGGL((conv_grouped_kernel<T, P, S, TH, ZINS>), grid, dim3(256),
                     0, grouped_stream(),
                     reinterpret_cast<const T*>(src.data_ptr()),
                     reinterpret_cast<const T*>(wp.data_ptr()),
                     reinterpret_cast<T*>(out.data_ptr()), d);
}

// The P = 64 stride-2 forward takes 4-row tiles: its 18 x 34 patch plus the
// 81 KB filter would not fit in LDS.
template <typename T>
void launch_grouped(const at::Tensor& src, const at::Tensor& wp,
                    at::Tensor& out, const GDims& d, int P, int stride,
                    bool zins) {
  if (P == 32) {
    if (zins) launch_grouped_t<T, 32, 1, 8, true>(src, wp, out, d);
    else if (stride == 1) launch_grouped_t<T, 32, 1, 8, false>(src, wp, out, d);
    else launch_grouped_t<T, 32, 2, 8, false>(src, wp, out, d);
  } else {
    if (zins) launch_grouped_t<T, 64, 1, 8, true>(src, wp, out, d);
    else if (stride == 1) launch_grouped_t<T, 64, 1, 8, false>(src, wp, out, d);
    else launch_grouped_t<T, 64, 2, 4, false>(src, wp, out, d);
  }
}

template <typename T, int P>
void launch_wgrad(const at::Tensor& dy, const at::Tensor& x,
                  at::Tensor& slab, const GDims& d, int stride, int splits) {
  const dim3 grid(d.C / P, splits);
  auto* kern = stride == 1 ? conv_grouped_wgrad_kernel<T, P, 1>
                           : conv_grouped_wgrad_kernel<T, P, 2>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, grouped_stream(),
                     reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     slab.data_ptr<float>(), d);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// (wp, wpT): the forward and the input-grad operand of a (C, Cg, 3, 3) filter.
std::tuple<at::Tensor, at::Tensor> conv_grouped_prep(at::Tensor w,
                                                     long groups) {
  TORCH_CHECK(w.is_cuda() && is_16bit(w) && w.dim() == 4 && w.size(2) == 3 &&
              w.size(3) == 3,
              "conv_grouped_prep expects a bf16 or fp16 (C, Cg, 3, 3) HIP "
              "filter");
  const long C = w.size(0);
  const int P = pack_width(C, groups);
  TORCH_CHECK(w.size(1) == C / groups, "conv_grouped_prep: filter is (",
              C, ", ", w.size(1), ", 3, 3) but groups is ", groups);
  auto both = at::empty({2, C / P, 9, P, P}, w.options().memory_format(
                                                 at::MemoryFormat::Contiguous));
  const long total = 9 * C * P;
  const int blocks = (int)std::min((total + 255) / 256, 2048L);
  auto* base = reinterpret_cast<unsigned short*>(both.data_ptr());
  hipLaunchKernelGGL(grouped_prep_kernel, dim3(blocks), dim3(256), 0,
                     grouped_stream(),
                     reinterpret_cast<const unsigned short*>(w.data_ptr()),
                     base, base + total, total, (int)(C / groups), P,
                     (long)w.stride(0), (long)w.stride(1), (long)w.stride(2),
                     (long)w.stride(3));
  return std::make_tuple(both[0], both[1]);
}

at::Tensor conv_grouped_fwd(at::Tensor x, at::Tensor wp, long stride) {
  check_act(x, "x");
  TORCH_CHECK(stride == 1 || stride == 2, "grouped conv: stride must be 1 or 2");
  const int P = check_packed(wp, x.size(1), x);
  GDims d{};
  d.Nb = x.size(0); d.C = x.size(1);
  d.SH = d.VH = x.size(2); d.SW = d.VW = x.size(3);
  d.OH = out_extent(d.SH, stride); d.OW = out_extent(d.SW, stride);
  auto y = at::empty({d.Nb, d.C, d.OH, d.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (x.scalar_type() == at::kHalf)
    launch_grouped<_Float16>(x, wp, y, d, P, (int)stride, false);
  else
    launch_grouped<__bf16>(x, wp, y, d, P, (int)stride, false);
  return y;
}

at::Tensor conv_grouped_dgrad(at::Tensor dy, at::Tensor wpT, long H, long W,
                              long stride) {
  check_act(dy, "dy");
  TORCH_CHECK(stride == 1 || stride == 2, "grouped conv: stride must be 1 or 2");
  TORCH_CHECK(H > 0 && W > 0 && dy.size(2) == out_extent(H, stride) &&
              dy.size(3) == out_extent(W, stride),
              "conv_grouped_dgrad: dy's extents do not belong to a ", H, " x ",
              W, " input at stride ", stride);
  const int P = check_packed(wpT, dy.size(1), dy);
  GDims d{};
  d.Nb = dy.size(0); d.C = dy.size(1);
  d.SH = dy.size(2); d.SW = dy.size(3);
  d.VH = d.OH = H; d.VW = d.OW = W;
  auto dx = at::empty({d.Nb, d.C, H, W},
                      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (dy.scalar_type() == at::kHalf)
    launch_grouped<_Float16>(dy, wpT, dx, d, P, 1, stride == 2);
  else
    launch_grouped<__bf16>(dy, wpT, dx, d, P, 1, stride == 2);
  return dx;
}

// splits: 0 = about one resident set of blocks; else that many (at most one
// per tile).
at::Tensor conv_grouped_wgrad(at::Tensor dy, at::Tensor x, long groups,
                              long stride, long splits) {
  check_act(dy, "dy");
  check_act(x, "x");
  check_same_16(dy, "dy", x, "x");
  TORCH_CHECK(stride == 1 || stride == 2, "grouped conv: stride must be 1 or 2");
  const long C = x.size(1);
  const int P = pack_width(C, groups);
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == C &&
              dy.size(2) == out_extent(x.size(2), stride) &&
              dy.size(3) == out_extent(x.size(3), stride),
              "conv_grouped_wgrad: dy does not belong to x at stride ", stride);
  TORCH_CHECK(splits >= 0, "conv_grouped_wgrad: splits must be >= 0");
  GDims d{};
  d.Nb = x.size(0); d.C = C;
  d.SH = d.VH = x.size(2); d.SW = d.VW = x.size(3);
  d.OH = dy.size(2); d.OW = dy.size(3);
  d.tiles_h = (d.OH + WTH - 1) / WTH;
  d.tiles_w = (d.OW + TW - 1) / TW;
  const long tiles = (long)d.Nb * d.tiles_h * d.tiles_w;
  TORCH_CHECK(tiles < (1L << 30), "conv_grouped_wgrad: too many tiles");
  const long packs = C / P;
  if (splits == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    splits = std::max(1L, 2 * cus / packs);
  }
  splits = std::min({splits, tiles, 65535L});
  const long split_stride = packs * 9 * P * P;
  auto slab = at::empty({splits * split_stride},
                        x.options().dtype(at::kFloat));
  if (x.scalar_type() == at::kHalf) {
    if (P == 32) launch_wgrad<_Float16, 32>(dy, x, slab, d, stride, splits);
    else launch_wgrad<_Float16, 64>(dy, x, slab, d, stride, splits);
  } else {
    if (P == 32) launch_wgrad<__bf16, 32>(dy, x, slab, d, stride, splits);
    else launch_wgrad<__bf16, 64>(dy, x, slab, d, stride, splits);
  }
  const long Cg = C / groups;
  auto dw = at::empty({C, Cg, 3, 3},
                      x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const long total = C * Cg * 9;
  const int blocks = (int)std::min((total + 255) / 256, 2048L);
  if (x.scalar_type() == at::kHalf)
    hipLaunchKernelGGL(grouped_wgrad_reduce_kernel<_Float16>, dim3(blocks),
                       dim3(256), 0, grouped_stream(),
                       slab.data_ptr<float>(),
                       reinterpret_cast<_Float16*>(dw.data_ptr()), total,
                       (int)Cg, P, (int)splits, split_stride);
  else
    hipLaunchKernelGGL(grouped_wgrad_reduce_kernel<__bf16>, dim3(blocks),
                       dim3(256), 0, grouped_stream(),
                       slab.data_ptr<float>(),
                       reinterpret_cast<__bf16*>(dw.data_ptr()), total,
                       (int)Cg, P, (int)splits, split_stride);
  return dw;
}
