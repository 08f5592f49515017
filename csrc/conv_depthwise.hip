// MI355X (gfx950/CDNA4) depthwise 3x3 convolution — NHWC bf16 or fp16, fp32
// accumulation, pad 1, stride 1 or 2, groups == in_channels == out_channels
// == C, C a multiple of 8. One channel per group leaves nothing for a matrix
// instruction to contract over, so this is VALU code bound by memory: every
// global and every LDS access of an activation is 16 bytes (8 channels).
//
// Work split (all three passes). A block of 256 threads owns a chunk of 64
// channels and a tile of output pixels. tid & 7 is the lane's group of 8
// consecutive channels, tid >> 3 one of 32 pixel slots. The last chunk may be
// ragged: lanes with c >= C stage zeros and store nothing.
//
// LDS. The block stages the halo patch of its tile, [image][row][col][64
// channels] with zeros outside the image, so an input element leaves HBM once
// per tile and a pixel's 8 lanes read 128 contiguous bytes. The filter chunk
// is read once through the tensor's strides into LDS as [9][64] and from
// there into 72 fp32 registers per lane. There is no prep launch.
//
// fwd / dgrad (conv_dw_kernel). A slot owns a column segment of VR output
// rows and walks the (VR-1)*s+3 patch rows under it once: each row's three
// pixels are unpacked to fp32 and feed every output row they are a tap of (a
// rolling window, unrolled). The stride-1 input grad is the same loop on dy
// with tap 8 - t. The stride-2 input grad is a gather: dx[ih][iw] sums the
// taps with (ih+1-r) and (iw+1-s) even, from a (TH/2+1) x (TW/2+1) patch of
// dy; pixels are dealt to slots by parity class so that a wave's lanes take
// the same taps wherever a tile has 32 pixels or more per image. dx is
// written in full.
//
// Tile variants <TH, TW, NI, VR> with NI * (TH/VR) * TW == 32 slots; NI > 1
// puts several images of one channel chunk into one block, each with its own
// halo, for the late small layers:
//   stride 1 (fwd, dgrad), stride-2 dgrad     stride-2 fwd, wgrad
//   out <= 4x4      4 x 4  x 8 images           4 x 4 x 4 images
//   out width <= 8  8 x 8  x 2 images           8 x 8 x 1
//   else            8 x 16 x 1                  8 x 8 x 1
// (the stride-2 patches are 4x the area; these keep a block under 42 KB).
//
// wgrad (conv_dw_wgrad_kernel + dw_wgrad_reduce_kernel). A block owns a chunk
// and a contiguous range of the (image group, tile) list. A lane keeps 9 x 8
// fp32 sums over the pixels its slot walks; dy comes straight from global
// memory (each element has one reader), x from the patch. The 32 slots are
// then folded through LDS in slot order and the block writes its fp32 row
// [split][9][C]; the reduce sums the splits in order and rounds once. No
// atomics, no memset: a result depends on (shape, splits) only.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int CHUNK = 64;   // channels per block
constexpr int LANES = 8;    // 16-byte lanes per pixel of a chunk
constexpr int SLOTS = 32;   // pixel slots per block

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

struct DwDims {
  int N, C;
  int SH, SW;    // extents of the staged tensor (x; dy for the input grad)
  int OH, OW;    // extents the tile grid covers (y; dx; dy for wgrad)
  int tiles_h, tiles_w;
  int groups;    // ceil(N / NI)
  long wsk, wsr, wss;   // filter strides of (C, 1, 3, 3), in elements
};

// Patch [NI][PH][PW][8 lanes] <- src rows r0.., cols c0.. of images n0..,
// channels c0ch.., zeros outside the image, the batch and the channels.
template <int NI, int PH, int PW>
__device__ __forceinline__ void stage_patch(u32x4* patch, const void* src,
                                            const DwDims& d, int n0, int r0,
                                            int c0, int c0ch) {
  const u32x4* s = reinterpret_cast<const u32x4*>(src);
  for (int e = threadIdx.x; e < NI * PH * PW * LANES; e += 256) {
    const int cl = e & 7;
    int pix = e >> 3;
    const int pc = pix % PW; pix /= PW;
    const int pr = pix % PH;
    const int n = n0 + pix / PH;
    const int r = r0 + pr, c = c0 + pc, ch = c0ch + cl * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n < d.N && r >= 0 && r < d.SH && c >= 0 && c < d.SW && ch < d.C)
      v = s[((((size_t)n * d.SH + r) * d.SW + c) * d.C + ch) >> 3];
    patch[e] = v;
  }
}

// wl [9][64] <- the chunk's filter, zeros past C; read through the strides.
template <typename T>
__device__ __forceinline__ void stage_filter(T* wl, const T* w,
                                             const DwDims& d, int c0ch) {
  for (int i = threadIdx.x; i < 9 * CHUNK; i += 256) {
    const int tap = i >> 6, c = c0ch + (i & 63);
    wl[i] = c < d.C ? w[c * d.wsk + (tap / 3) * d.wsr + (tap % 3) * d.wss]
                    : (T)0.f;
  }
}

// ---------------------------------------------------------------------------
// fwd / dgrad
// ---------------------------------------------------------------------------
template <typename T, int S, bool DGRAD, int TH, int TW, int NI, int VR>
__global__ __launch_bounds__(256)
void conv_dw_kernel(const T* __restrict__ src, const T* __restrict__ w,
                    T* __restrict__ out, DwDims d) {
  constexpr bool GATHER = DGRAD && S == 2;
  constexpr int PH = GATHER ? TH / 2 + 1 : (TH - 1) * S + 3;
  constexpr int PW = GATHER ? TW / 2 + 1 : (TW - 1) * S + 3;
  static_assert(TH % 2 == 0 && TW % 2 == 0, "the gather wants even origins");
  static_assert(GATHER || NI * (TH / VR) * TW == SLOTS, "32 slots per block");
  static_assert(!GATHER || (NI * TH * TW) % SLOTS == 0, "whole slots");
  __shared__ u32x4 patch[NI * PH * PW * LANES];
  __shared__ u32x4 wl[9 * LANES];

  int b = blockIdx.x;
  const int tw_i = b % d.tiles_w; b /= d.tiles_w;
  const int th_i = b % d.tiles_h;
  const int n0 = (b / d.tiles_h) * NI;
  const int c0ch = blockIdx.y * CHUNK;
  const int o_r0 = th_i * TH, o_c0 = tw_i * TW;
  const int cl = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int ch = c0ch + cl * 8;

  stage_filter<T>(reinterpret_cast<T*>(wl), w, d, c0ch);
  if (GATHER) stage_patch<NI, PH, PW>(patch, src, d, n0, o_r0 / 2, o_c0 / 2,
                                      c0ch);
  else stage_patch<NI, PH, PW>(patch, src, d, n0, o_r0 * S - 1, o_c0 * S - 1,
                               c0ch);
  __syncthreads();

  float wr[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t) unpack8<T>(wl[t * LANES + cl], wr[t]);

  if constexpr (!GATHER) {
    const int col = slot % TW;
    const int seg = (slot / TW) % (TH / VR);
    const int img = slot / (TW * (TH / VR));
    const u32x4* p = patch + ((img * PH + seg * VR * S) * PW + col * S) *
                                 LANES + cl;
    float acc[VR][8];
#pragma unroll
    for (int j = 0; j < VR; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int pr = 0; pr < (VR - 1) * S + 3; ++pr) {
      float v[3][8];
#pragma unroll
      for (int s = 0; s < 3; ++s)
        unpack8<T>(p[(pr * PW + s) * LANES], v[s]);
#pragma unroll
      for (int j = 0; j < VR; ++j) {
        const int r = pr - j * S;
        if (r < 0 || r > 2) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int t = DGRAD ? 8 - (r * 3 + s) : r * 3 + s;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[j][i] = fmaf(v[s][i], wr[t][i], acc[j][i]);
        }
      }
    }
    const int n = n0 + img, oc = o_c0 + col;
    if (n < d.N && oc < d.OW && ch < d.C) {
#pragma unroll
      for (int j = 0; j < VR; ++j) {
        const int orow = o_r0 + seg * VR + j;
        if (orow < d.OH)
          reinterpret_cast<u32x4*>(out)[((((size_t)n * d.OH + orow) * d.OW +
                                          oc) * d.C + ch) >> 3] =
              pack8<T>(acc[j]);
      }
    }
  } else {
    constexpr int PER_IMG = TH * TW, PER_CLS = PER_IMG / 4;
#pragma unroll
    for (int k = 0; k < NI * PER_IMG / SLOTS; ++k) {
      const int pidx = slot + SLOTS * k;
      const int img = pidx / PER_IMG, q = pidx % PER_IMG;
      const int cls = q / PER_CLS, qq = q % PER_CLS;
      const int row = 2 * (qq / (TW / 2)) + (cls >> 1);
      const int col = 2 * (qq % (TW / 2)) + (cls & 1);
      float acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.f;
      // tile origins are even, so row and col carry the parity of ih and iw;
      // a dy row or column past the image is a zero of the patch
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if ((row + 1 - r) & 1) continue;
        const int lr = (row + 1 - r) >> 1;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          if ((col + 1 - s) & 1) continue;
          const int lc = (col + 1 - s) >> 1;
          float v[8];
          unpack8<T>(patch[((img * PH + lr) * PW + lc) * LANES + cl], v);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[i] = fmaf(v[i], wr[r * 3 + s][i], acc[i]);
        }
      }
      const int n = n0 + img, orow = o_r0 + row, oc = o_c0 + col;
      if (n < d.N && orow < d.OH && oc < d.OW && ch < d.C)
        reinterpret_cast<u32x4*>(out)[((((size_t)n * d.OH + orow) * d.OW +
                                        oc) * d.C + ch) >> 3] = pack8<T>(acc);
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------
// grid (splits, chunks). d.OH, d.OW are dy's extents, d.SH, d.SW x's.
template <typename T, int S, int TH, int TW, int NI>
__global__ __launch_bounds__(256)
void conv_dw_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                          float* __restrict__ slab, DwDims d) {
  constexpr int PH = (TH - 1) * S + 3, PW = (TW - 1) * S + 3;
  constexpr int PATCH = NI * PH * PW * LANES;
  constexpr int FOLD = 3 * SLOTS * CHUNK / 4;   // three taps of fp32, in 16 B
  static_assert((NI * TH * TW) % SLOTS == 0, "whole slots");
  __shared__ u32x4 smem[PATCH > FOLD ? PATCH : FOLD];

  const int c0ch = blockIdx.y * CHUNK;
  const int cl = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int ch = c0ch + cl * 8;
  const long work = (long)d.groups * d.tiles_h * d.tiles_w;
  const long begin = work * blockIdx.x / gridDim.x;
  const long end = work * (blockIdx.x + 1) / gridDim.x;

  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[t][i] = 0.f;

  for (long item = begin; item < end; ++item) {
    long b = item;
    const int tw_i = (int)(b % d.tiles_w); b /= d.tiles_w;
    const int th_i = (int)(b % d.tiles_h);
    const int n0 = (int)(b / d.tiles_h) * NI;
    const int o_r0 = th_i * TH, o_c0 = tw_i * TW;
    __syncthreads();   // the previous item's readers are done
    stage_patch<NI, PH, PW>(smem, x, d, n0, o_r0 * S - 1, o_c0 * S - 1, c0ch);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NI * TH * TW / SLOTS; ++k) {
      const int pidx = slot + SLOTS * k;
      const int img = pidx / (TH * TW), q = pidx % (TH * TW);
      const int row = q / TW, col = q % TW;
      const int n = n0 + img, orow = o_r0 + row, oc = o_c0 + col;
      if (n < d.N && orow < d.OH && oc < d.OW && ch < d.C) {
        float g[8];
        unpack8<T>(reinterpret_cast<const u32x4*>(dy)[
                       ((((size_t)n * d.OH + orow) * d.OW + oc) * d.C + ch) >>
                       3], g);
        const u32x4* p = smem + ((img * PH + row * S) * PW + col * S) * LANES +
                         cl;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            float v[8];
            unpack8<T>(p[(r * PW + s) * LANES], v);
#pragma unroll
            for (int i = 0; i < 8; ++i)
              acc[r * 3 + s][i] = fmaf(g[i], v[i], acc[r * 3 + s][i]);
          }
      }
    }
  }

  // fold the 32 slots in slot order, three taps per pass: f[tap][slot][64]
  float* f = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
      f32x4* dst = reinterpret_cast<f32x4*>(
          f + (tt * SLOTS + slot) * CHUNK + cl * 8);
      const float* a = acc[pass * 3 + tt];
      dst[0] = f32x4{a[0], a[1], a[2], a[3]};
      dst[1] = f32x4{a[4], a[5], a[6], a[7]};
    }
    __syncthreads();
    if (threadIdx.x < 3 * CHUNK) {
      const int tt = threadIdx.x >> 6, cc = threadIdx.x & 63;
      float sum = 0.f;
      for (int s = 0; s < SLOTS; ++s) sum += f[(tt * SLOTS + s) * CHUNK + cc];
      if (c0ch + cc < d.C)
        slab[((size_t)blockIdx.x * 9 + pass * 3 + tt) * d.C + c0ch + cc] = sum;
    }
  }
}

// dw (C, 1, 3, 3) contiguous <- slab [splits][9][C], splits summed in order.
template <typename T>
__global__ __launch_bounds__(256)
void dw_wgrad_reduce_kernel(const float* __restrict__ slab, T* __restrict__ dw,
                            int C, int splits) {
  const int total = 9 * C;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total;
       o += gridDim.x * 256) {
    const int tap = o / C, c = o % C;   // coalesced reads of the slab
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slab[((size_t)z * 9 + tap) * C + c];
    dw[c * 9 + tap] = (T)s;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
hipStream_t dw_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline bool is_16bit(const at::Tensor& t) {
  return t.scalar_type() == at::ScalarType::BFloat16 ||
         t.scalar_type() == at::ScalarType::Half;
}

inline void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && is_16bit(t), "depthwise conv: ", name,
              " must be a bf16 or fp16 HIP tensor, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.numel() > 0 &&
              t.is_contiguous(at::MemoryFormat::ChannelsLast),
              "depthwise conv: ", name, " must be 4-D channels_last");
  TORCH_CHECK(t.size(1) % 8 == 0, "depthwise conv: C must be a multiple of 8, "
              "got ", t.size(1));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "depthwise conv: ", name, " must be 16-byte aligned");
  TORCH_CHECK(t.size(0) < (1L << 24) && t.size(2) < (1L << 24) &&
              t.size(3) < (1L << 24) && t.size(1) < (1L << 24),
              "depthwise conv: ", name, " has an extent of 2^24 or more");
}

inline void check_same_16(const at::Tensor& a, const char* an,
                          const at::Tensor& b, const char* bn) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "depthwise conv: ", an,
              " is ", a.scalar_type(), " but ", bn, " is ", b.scalar_type(),
              ": the 16-bit operands of a conv call must share one dtype");
}

inline void check_stride(long stride) {
  TORCH_CHECK(stride == 1 || stride == 2,
              "depthwise conv: stride must be 1 or 2, got ", stride);
}

inline void check_filter(const at::Tensor& w, const at::Tensor& act) {
  TORCH_CHECK(w.is_cuda() && is_16bit(w), "depthwise conv: the filter must be "
              "a bf16 or fp16 HIP tensor, got ", w.scalar_type());
  check_same_16(act, "the activation", w, "the filter");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == act.size(1) && w.size(1) == 1 &&
              w.size(2) == 3 && w.size(3) == 3,
              "depthwise conv: the filter must be (C, 1, 3, 3) with C = ",
              act.size(1), ", got ", w.sizes());
}

inline long out_extent(long in, long stride) { return (in - 1) / stride + 1; }

// 0: 4x4 tiles of several images, 1: 8x8, 2: the wide tile
inline int tile_class(int OH, int OW) {
  if (OH <= 4 && OW <= 4) return 0;
  return OW <= 8 ? 1 : 2;
}

inline void set_grid(DwDims& d, int TH, int TW, int NI) {
  d.tiles_h = (d.OH + TH - 1) / TH;
  d.tiles_w = (d.OW + TW - 1) / TW;
  d.groups = (d.N + NI - 1) / NI;
}

template <typename T, int S, bool DGRAD, int TH, int TW, int NI, int VR>
void launch_dw_t(const at::Tensor& src, const at::Tensor& w, at::Tensor& out,
                 DwDims d) {
  set_grid(d, TH, TW, NI);
  const long blocks = (long)d.groups * d.tiles_h * d.tiles_w;
  TORCH_CHECK(blocks < (1L << 31), "depthwise conv: too many tiles");
  const dim3 grid((unsigned)blocks, (d.C + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL((conv_dw_kernel<T, S, DGRAD, TH, TW, NI, VR>), grid,
                     dim3(256), 0, dw_stream(),
                     reinterpret_cast<const T*>(src.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(out.data_ptr()), d);
}

template <typename T>
void launch_dw(const at::Tensor& src, const at::Tensor& w, at::Tensor& out,
               const DwDims& d, int stride, bool dgrad) {
  const int cls = tile_class(d.OH, d.OW);
  if (stride == 2 && !dgrad) {
    if (cls == 0) launch_dw_t<T, 2, false, 4, 4, 4, 2>(src, w, out, d);
    else launch_dw_t<T, 2, false, 8, 8, 1, 2>(src, w, out, d);
  } else if (stride == 2) {
    if (cls == 0) launch_dw_t<T, 2, true, 4, 4, 8, 4>(src, w, out, d);
    else if (cls == 1) launch_dw_t<T, 2, true, 8, 8, 2, 4>(src, w, out, d);
    else launch_dw_t<T, 2, true, 8, 16, 1, 4>(src, w, out, d);
  } else if (dgrad) {
    if (cls == 0) launch_dw_t<T, 1, true, 4, 4, 8, 4>(src, w, out, d);
    else if (cls == 1) launch_dw_t<T, 1, true, 8, 8, 2, 4>(src, w, out, d);
    else launch_dw_t<T, 1, true, 8, 16, 1, 4>(src, w, out, d);
  } else {
    if (cls == 0) launch_dw_t<T, 1, false, 4, 4, 8, 4>(src, w, out, d);
    else if (cls == 1) launch_dw_t<T, 1, false, 8, 8, 2, 4>(src, w, out, d);
    else launch_dw_t<T, 1, false, 8, 16, 1, 4>(src, w, out, d);
  }
}

template <typename T, int S, int TH, int TW, int NI>
void launch_wgrad_t(const at::Tensor& dy, const at::Tensor& x,
                    at::Tensor& slab, const DwDims& d, int splits) {
  const dim3 grid(splits, (d.C + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL((conv_dw_wgrad_kernel<T, S, TH, TW, NI>), grid, dim3(256),
                     0, dw_stream(), reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     slab.data_ptr<float>(), d);
}

template <typename T>
void launch_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& slab,
                  const DwDims& d, int stride, int cls, int splits) {
  if (stride == 2) {
    if (cls == 0) launch_wgrad_t<T, 2, 4, 4, 4>(dy, x, slab, d, splits);
    else launch_wgrad_t<T, 2, 8, 8, 1>(dy, x, slab, d, splits);
  } else {
    if (cls == 0) launch_wgrad_t<T, 1, 4, 4, 8>(dy, x, slab, d, splits);
    else if (cls == 1) launch_wgrad_t<T, 1, 8, 8, 2>(dy, x, slab, d, splits);
    else launch_wgrad_t<T, 1, 8, 16, 1>(dy, x, slab, d, splits);
  }
}

inline void set_filter_strides(DwDims& d, const at::Tensor& w) {
  d.wsk = w.stride(0); d.wsr = w.stride(2); d.wss = w.stride(3);
}

}  // namespace

at::Tensor conv_dw_fwd(at::Tensor x, at::Tensor w, long stride) {
  check_act(x, "x");
  check_filter(w, x);
  check_stride(stride);
  DwDims d{};
  d.N = x.size(0); d.C = x.size(1);
  d.SH = x.size(2); d.SW = x.size(3);
  d.OH = out_extent(d.SH, stride); d.OW = out_extent(d.SW, stride);
  set_filter_strides(d, w);
  auto y = at::empty({d.N, d.C, d.OH, d.OW},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (x.scalar_type() == at::kHalf)
    launch_dw<_Float16>(x, w, y, d, (int)stride, false);
  else
    launch_dw<__bf16>(x, w, y, d, (int)stride, false);
  return y;
}

at::Tensor conv_dw_dgrad(at::Tensor dy, at::Tensor w, long H, long W,
                         long stride) {
  check_act(dy, "dy");
  check_filter(w, dy);
  check_stride(stride);
  TORCH_CHECK(H > 0 && W > 0 && H < (1L << 24) && W < (1L << 24) &&
              dy.size(2) == out_extent(H, stride) &&
              dy.size(3) == out_extent(W, stride),
              "depthwise conv: dy's extents do not belong to a ", H, " x ", W,
              " input at stride ", stride);
  DwDims d{};
  d.N = dy.size(0); d.C = dy.size(1);
  d.SH = dy.size(2); d.SW = dy.size(3);
  d.OH = H; d.OW = W;
  set_filter_strides(d, w);
  auto dx = at::empty({d.N, d.C, H, W},
                      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (dy.scalar_type() == at::kHalf)
    launch_dw<_Float16>(dy, w, dx, d, (int)stride, true);
  else
    launch_dw<__bf16>(dy, w, dx, d, (int)stride, true);
  return dx;
}

// splits: 0 = about four blocks per CU over all chunks, at most one per work
// item; a positive count is taken as it is (blocks past the work write zeros).
at::Tensor conv_dw_wgrad(at::Tensor dy, at::Tensor x, long stride,
                         long splits) {
  check_act(dy, "dy");
  check_act(x, "x");
  check_same_16(dy, "dy", x, "x");
  check_stride(stride);
  const long C = x.size(1);
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == C &&
              dy.size(2) == out_extent(x.size(2), stride) &&
              dy.size(3) == out_extent(x.size(3), stride),
              "depthwise conv: dy's extents do not belong to a ", x.size(2),
              " x ", x.size(3), " input at stride ", stride);
  TORCH_CHECK(splits >= 0 && splits <= 65535,
              "depthwise conv: splits must be in 0..65535, got ", splits);
  DwDims d{};
  d.N = x.size(0); d.C = C;
  d.SH = x.size(2); d.SW = x.size(3);
  d.OH = dy.size(2); d.OW = dy.size(3);
  const int cls = tile_class(d.OH, d.OW);
  if (cls == 0) set_grid(d, 4, 4, stride == 2 ? 4 : 8);
  else if (cls == 1 || stride == 2) set_grid(d, 8, 8, stride == 2 ? 1 : 2);
  else set_grid(d, 8, 16, 1);
  const long work = (long)d.groups * d.tiles_h * d.tiles_w;
  const long chunks = (C + CHUNK - 1) / CHUNK;
  if (splits == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    splits = std::min(std::max(1L, 4 * cus / chunks), std::min(work, 65535L));
  }
  auto slab = at::empty({splits, 9, C}, x.options().dtype(at::kFloat));
  auto dw = at::empty({C, 1, 3, 3}, x.options().memory_format(
                                        at::MemoryFormat::Contiguous));
  const int rblocks = (int)std::min((9 * C + 255) / 256, 2048L);
  if (x.scalar_type() == at::kHalf) {
    launch_wgrad<_Float16>(dy, x, slab, d, (int)stride, cls, (int)splits);
    hipLaunchKernelGGL(dw_wgrad_reduce_kernel<_Float16>, dim3(rblocks),
                       dim3(256), 0, dw_stream(), slab.data_ptr<float>(),
                       reinterpret_cast<_Float16*>(dw.data_ptr()), (int)C,
                       (int)splits);
  } else {
    launch_wgrad<__bf16>(dy, x, slab, d, (int)stride, cls, (int)splits);
    hipLaunchKernelGGL(dw_wgrad_reduce_kernel<__bf16>, dim3(rblocks),
                       dim3(256), 0, dw_stream(), slab.data_ptr<float>(),
                       reinterpret_cast<__bf16*>(dw.data_ptr()), (int)C,
                       (int)splits);
  }
  return dw;
}
