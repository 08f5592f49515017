// MI355X (gfx950/CDNA4) depthwise KxK convolution, K in {5, 7, 9} — NHWC bf16
// or fp16, fp32 accumulation, stride 1, pad K/2, groups == in_channels ==
// out_channels == C, C a multiple of 8: the large-kernel depthwise layers of
// ConvMixer (and of ConvNeXt, MobileNet-v3, EfficientNet). VALU code like the
// 3x3 kernels of conv_depthwise.hip, but at 2 K^2 flops per element it is the
// fp32 FMA rate, not memory, that bounds K = 7 and 9, and neither K^2 x 8
// filter registers nor K^2 LDS reads per output are affordable. So the work
// split is its own.
//
// Lane geometry (the family's). A block of 256 threads owns a chunk of 64
// channels and an 8 x 16 tile of pixels of one image. tid & 7 is the lane's
// group of 8 consecutive channels, so every global and LDS access of an
// activation is 16 bytes; tid >> 3 is one of 32 pixel slots. A ragged last
// chunk is predicated: lanes with c >= C stage zeros and store nothing.
// grid = (images x tiles, chunks).
//
// LDS. The (8+K-1) x (16+K-1) halo patch of the tile, [row][col][64 channels]
// with zeros outside the image: 30 / 38.5 / 48 KB at K = 5 / 7 / 9. Where it
// fits in 64 KB the row pitch is padded to an odd pixel count, so that slots
// one patch row apart (the 8 slots of a wave) alternate between the two
// 128-byte halves of the banks. The chunk's filter is read once through the
// tensor's strides into LDS as [K*K][64] 16-bit values. No prep launch.
//
// fwd / dgrad (conv_dwk_kernel). Slot = (row of the tile, run of 4 outputs
// along W); wave w holds run w of all 8 rows. Per filter row the slot takes
// that row's K x 8 weights into registers, then walks the K+3 patch pixels
// under its run once: a pixel is unpacked once and multiplied into every
// output of the run it is a tap of. That is K(K+3)/4 LDS vectors per output
// instead of K^2 (27 instead of 81 at K = 9), 32 accumulators and one filter
// row in registers. Accumulators, pixels and weights are float pairs, so the
// FMAs are the packed v_pk_fma_f32. The input grad is the same kernel on dy
// with tap K*K-1-t. Outputs are written in full with 16-byte stores.
//
// wgrad (conv_dwk_wgrad_kernel + dwk_wgrad_reduce_kernel). A block owns a
// chunk and a contiguous range of the (image, tile) list; per item it stages
// the x patch and the dy tile (zeros outside the image) in LDS. The K^2 x 8
// sums of a lane group do not fit a lane, so the filter rows are dealt to the
// waves: wave w owns the rows r = w, w+4, w+8 below K (at most 3 x K x 8 =
// 216 fp32 sums per lane), and its 8 slots each walk one row of the tile, dy
// pixel by pixel against the K x pixels around it (the rolling window again:
// each x pixel is unpacked once per filter row). At the end the 8 slots of a
// wave are folded through LDS in slot order, one filter column per pass, and
// the block writes its row of the fp32 slab [split][K*K][C]; the reduce sums
// the splits in order and rounds once. No atomics, no memset: a result
// depends on (shape, splits) only.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int CHUNK = 64;   // channels per block
constexpr int LANES = 8;    // 16-byte lanes per pixel of a chunk
constexpr int TH = 8, TW = 16;   // the tile
constexpr int RUN = 4;      // consecutive outputs of a fwd / dgrad slot
constexpr int LDS_LIMIT = 65536;

template <typename T>
__device__ __forceinline__ void unpack8(u32x4 v, f32x2 (&f)[4]) {
  typedef __attribute__((ext_vector_type(8))) T x8;
  const x8 e = __builtin_bit_cast(x8, v);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    f[i] = f32x2{(float)e[2 * i], (float)e[2 * i + 1]};
}

template <typename T>
__device__ __forceinline__ u32x4 pack8(const f32x2 (&f)[4]) {
  typedef __attribute__((ext_vector_type(8))) T x8;
  x8 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[2 * i] = (T)f[i].x;
    e[2 * i + 1] = (T)f[i].y;
  }
  return __builtin_bit_cast(u32x4, e);
}

struct DwkDims {
  int N, C, H, W;   // stride 1, pad K/2: every tensor has these extents
  int tiles_h, tiles_w;
  long wsk, wsr, wss;   // filter strides of (C, 1, K, K), in elements
};

// dst [PH][PITCH][8 lanes] <- src rows r0.., cols c0.. (PW of them) of image
// n, channels c0ch.., zeros outside the image and the channels.
template <int PH, int PW, int PITCH>
__device__ __forceinline__ void stage_patch(u32x4* dst, const void* src,
                                            const DwkDims& d, int n, int r0,
                                            int c0, int c0ch) {
  const u32x4* s = reinterpret_cast<const u32x4*>(src);
  for (int e = threadIdx.x; e < PH * PW * LANES; e += 256) {
    const int cl = e & 7, pix = e >> 3;
    const int pc = pix % PW, pr = pix / PW;
    const int r = r0 + pr, c = c0 + pc, ch = c0ch + cl * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r >= 0 && r < d.H && c >= 0 && c < d.W && ch < d.C)
      v = s[((((size_t)n * d.H + r) * d.W + c) * d.C + ch) >> 3];
    dst[(pr * PITCH + pc) * LANES + cl] = v;
  }
}

// patch row pitch in pixels: odd where the block's LDS stays within 64 KB
constexpr int patch_pitch(int K, int other_bytes) {
  const int ph = TH + K - 1, pw = TW + K - 1;
  return ph * (pw | 1) * LANES * 16 + other_bytes <= LDS_LIMIT ? (pw | 1) : pw;
}

// ---------------------------------------------------------------------------
// fwd / dgrad
// ---------------------------------------------------------------------------
template <typename T, int K, bool DGRAD>
__global__ __launch_bounds__(256)
void conv_dwk_kernel(const T* __restrict__ src, const T* __restrict__ w,
                     T* __restrict__ out, DwkDims d) {
  constexpr int PH = TH + K - 1, PW = TW + K - 1;
  constexpr int PITCH = patch_pitch(K, K * K * LANES * 16);
  static_assert((TH * TW / RUN) * LANES == 256, "one run per slot");
  static_assert((PH * PITCH + K * K) * LANES * 16 <= LDS_LIMIT, "LDS");
  __shared__ u32x4 patch[PH * PITCH * LANES];
  __shared__ u32x4 wl[K * K * LANES];   // [K*K][64] of T

  int b = blockIdx.x;
  const int tw_i = b % d.tiles_w; b /= d.tiles_w;
  const int th_i = b % d.tiles_h;
  const int n = b / d.tiles_h;
  const int c0ch = blockIdx.y * CHUNK;
  const int o_r0 = th_i * TH, o_c0 = tw_i * TW;
  const int cl = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int ch = c0ch + cl * 8;

  T* wlt = reinterpret_cast<T*>(wl);
  for (int i = threadIdx.x; i < K * K * CHUNK; i += 256) {
    const int tap = i >> 6, c = c0ch + (i & 63);
    wlt[i] = c < d.C ? w[c * d.wsk + (tap / K) * d.wsr + (tap % K) * d.wss]
                     : (T)0.f;
  }
  stage_patch<PH, PW, PITCH>(patch, src, d, n, o_r0 - K / 2, o_c0 - K / 2,
                             c0ch);
  __syncthreads();

  const int row = slot & 7, run = slot >> 3;   // a wave: one run, 8 rows
  const u32x4* p = patch + (row * PITCH + run * RUN) * LANES + cl;
  f32x2 acc[RUN][4];
#pragma unroll
  for (int j = 0; j < RUN; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x2{0.f, 0.f};

  // one filter row per trip; unrolled, the loads of all K rows are hoisted
  // and the registers run out
#pragma unroll 1
  for (int r = 0; r < K; ++r) {
    f32x2 wr[K][4];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int t = DGRAD ? K * K - 1 - (r * K + s) : r * K + s;
      unpack8<T>(wl[t * LANES + cl], wr[s]);
    }
#pragma unroll
    for (int pp = 0; pp < K + RUN - 1; ++pp) {
      f32x2 v[4];
      unpack8<T>(p[(r * PITCH + pp) * LANES], v);
#pragma unroll
      for (int j = 0; j < RUN; ++j) {
        const int s = pp - j;
        if (s < 0 || s >= K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[j][i] = __builtin_elementwise_fma(v[i], wr[s][i], acc[j][i]);
      }
    }
  }

  const int orow = o_r0 + row;
  if (orow < d.H && ch < d.C) {
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
      const int oc = o_c0 + run * RUN + j;
      if (oc < d.W)
        reinterpret_cast<u32x4*>(out)[((((size_t)n * d.H + orow) * d.W + oc) *
                                       d.C + ch) >> 3] = pack8<T>(acc[j]);
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------
// grid (splits, chunks).
template <typename T, int K>
__global__ __launch_bounds__(256)
void conv_dwk_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                           float* __restrict__ slab, DwkDims d) {
  constexpr int PH = TH + K - 1, PW = TW + K - 1;
  constexpr int TILE = TH * TW * LANES;            // the dy tile, in 16 B
  constexpr int PITCH = patch_pitch(K, TILE * 16);
  constexpr int PATCH = PH * PITCH * LANES;
  constexpr int NR = (K + 3) / 4;                  // filter rows of wave 0
  static_assert((PATCH + TILE) * 16 <= LDS_LIMIT, "LDS");
  static_assert(K * 8 * CHUNK * 4 <= (PATCH + TILE) * 16, "the fold fits");
  __shared__ u32x4 smem[PATCH + TILE];
  u32x4* dyt = smem + PATCH;

  const int c0ch = blockIdx.y * CHUNK;
  const int cl = threadIdx.x & 7;
  const int row = (threadIdx.x >> 3) & 7;   // the slot's row of the tile
  const int wv = threadIdx.x >> 6;          // filter rows wv, wv + 4, wv + 8
  const long work = (long)d.N * d.tiles_h * d.tiles_w;
  const long begin = work * blockIdx.x / gridDim.x;
  const long end = work * (blockIdx.x + 1) / gridDim.x;

  f32x2 acc[NR][K][4];
#pragma unroll
  for (int ri = 0; ri < NR; ++ri)
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ri][s][i] = f32x2{0.f, 0.f};

  for (long item = begin; item < end; ++item) {
    long b = item;
    const int tw_i = (int)(b % d.tiles_w); b /= d.tiles_w;
    const int th_i = (int)(b % d.tiles_h);
    const int n = (int)(b / d.tiles_h);
    const int o_r0 = th_i * TH, o_c0 = tw_i * TW;
    __syncthreads();   // the previous item's readers are done
    stage_patch<PH, PW, PITCH>(smem, x, d, n, o_r0 - K / 2, o_c0 - K / 2,
                               c0ch);
    stage_patch<TH, TW, TW>(dyt, dy, d, n, o_r0, o_c0, c0ch);
    __syncthreads();
    const u32x4* g_p = dyt + row * TW * LANES + cl;
#pragma unroll
    for (int ri = 0; ri < NR; ++ri) {
      const int r = wv + 4 * ri;
      if (r >= K) continue;   // the same for a whole wave
      const u32x4* x_p = smem + (row + r) * PITCH * LANES + cl;
      f32x2 xw[PW][4];        // the window: K of them are live at a time
#pragma unroll
      for (int pc = 0; pc < K - 1; ++pc) unpack8<T>(x_p[pc * LANES], xw[pc]);
      // the next column's two vectors are in flight during this one's FMAs;
      // the fence keeps the scheduler from hoisting the whole row's loads
      u32x4 x_raw = x_p[(K - 1) * LANES], g_raw = g_p[0];
#pragma unroll
      for (int col = 0; col < TW; ++col) {
        f32x2 g[4];
        unpack8<T>(x_raw, xw[col + K - 1]);
        unpack8<T>(g_raw, g);
        if (col + 1 < TW) {
          x_raw = x_p[(col + K) * LANES];
          g_raw = g_p[(col + 1) * LANES];
        }
#pragma unroll
        for (int s = 0; s < K; ++s)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[ri][s][i] = __builtin_elementwise_fma(g[i], xw[col + s][i],
                                                      acc[ri][s][i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // fold the 8 slots of every wave in slot order, one filter column s per
  // pass: f[filter row][slot][64]
  float* f = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int s = 0; s < K; ++s) {
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < NR; ++ri) {
      const int r = wv + 4 * ri;
      if (r >= K) continue;
      f32x4* dst = reinterpret_cast<f32x4*>(f + (r * 8 + row) * CHUNK + cl * 8);
      const f32x2* a = acc[ri][s];
      dst[0] = f32x4{a[0].x, a[0].y, a[1].x, a[1].y};
      dst[1] = f32x4{a[2].x, a[2].y, a[3].x, a[3].y};
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K * CHUNK; t += 256) {
      const int r = t >> 6, cc = t & 63;
      float sum = 0.f;
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) sum += f[(r * 8 + sl) * CHUNK + cc];
      if (c0ch + cc < d.C)
        slab[((size_t)blockIdx.x * K * K + r * K + s) * d.C + c0ch + cc] = sum;
    }
  }
}

// dw (C, 1, K, K) contiguous <- slab [splits][K*K][C], splits summed in order.
template <typename T>
__global__ __launch_bounds__(256)
void dwk_wgrad_reduce_kernel(const float* __restrict__ slab,
                             T* __restrict__ dw, int C, int KK, int splits) {
  const int total = KK * C;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total;
       o += gridDim.x * 256) {
    const int tap = o / C, c = o % C;   // coalesced reads of the slab
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slab[((size_t)z * KK + tap) * C + c];
    dw[(size_t)c * KK + tap] = (T)s;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
hipStream_t dwk_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline bool is_16bit(const at::Tensor& t) {
  return t.scalar_type() == at::ScalarType::BFloat16 ||
         t.scalar_type() == at::ScalarType::Half;
}

inline void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && is_16bit(t), "depthwise KxK conv: ", name,
              " must be a bf16 or fp16 HIP tensor, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.numel() > 0 &&
              t.is_contiguous(at::MemoryFormat::ChannelsLast),
              "depthwise KxK conv: ", name, " must be 4-D channels_last");
  TORCH_CHECK(t.size(1) % 8 == 0, "depthwise KxK conv: C must be a multiple "
              "of 8, got ", t.size(1));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "depthwise KxK conv: ", name, " must be 16-byte aligned");
  TORCH_CHECK(t.size(0) < (1L << 24) && t.size(2) < (1L << 24) &&
              t.size(3) < (1L << 24) && t.size(1) < (1L << 24),
              "depthwise KxK conv: ", name, " has an extent of 2^24 or more");
}

inline void check_same_16(const at::Tensor& a, const char* an,
                          const at::Tensor& b, const char* bn) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "depthwise KxK conv: ", an,
              " is ", a.scalar_type(), " but ", bn, " is ", b.scalar_type(),
              ": the 16-bit operands of a conv call must share one dtype");
}

inline void check_k(long K) {
  TORCH_CHECK(K == 5 || K == 7 || K == 9,
              "depthwise KxK conv: K must be 5, 7 or 9, got ", K);
}

inline void check_filter(const at::Tensor& w, const at::Tensor& act) {
  TORCH_CHECK(w.is_cuda() && is_16bit(w), "depthwise KxK conv: the filter "
              "must be a bf16 or fp16 HIP tensor, got ", w.scalar_type());
  check_same_16(act, "the activation", w, "the filter");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == act.size(1) && w.size(1) == 1 &&
              w.size(2) == w.size(3),
              "depthwise KxK conv: the filter must be (C, 1, K, K) with C = ",
              act.size(1), ", got ", w.sizes());
  check_k(w.size(2));
}

inline DwkDims make_dims(const at::Tensor& act) {
  DwkDims d{};
  d.N = act.size(0); d.C = act.size(1);
  d.H = act.size(2); d.W = act.size(3);
  d.tiles_h = (d.H + TH - 1) / TH;
  d.tiles_w = (d.W + TW - 1) / TW;
  return d;
}

template <typename T, int K, bool DGRAD>
void launch_dwk_k(const at::Tensor& src, const at::Tensor& w, at::Tensor& out,
                  const DwkDims& d) {
  const long blocks = (long)d.N * d.tiles_h * d.tiles_w;
  TORCH_CHECK(blocks < (1L << 31), "depthwise KxK conv: too many tiles");
  const dim3 grid((unsigned)blocks, (d.C + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL((conv_dwk_kernel<T, K, DGRAD>), grid, dim3(256), 0,
                     dwk_stream(), reinterpret_cast<const T*>(src.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(out.data_ptr()), d);
}

template <typename T, bool DGRAD>
void launch_dwk(const at::Tensor& src, const at::Tensor& w, at::Tensor& out,
                const DwkDims& d, int K) {
  if (K == 5) launch_dwk_k<T, 5, DGRAD>(src, w, out, d);
  else if (K == 7) launch_dwk_k<T, 7, DGRAD>(src, w, out, d);
  else launch_dwk_k<T, 9, DGRAD>(src, w, out, d);
}

template <bool DGRAD>
at::Tensor run_dwk(const at::Tensor& src, const char* name,
                   const at::Tensor& w) {
  check_act(src, name);
  check_filter(w, src);
  DwkDims d = make_dims(src);
  d.wsk = w.stride(0); d.wsr = w.stride(2); d.wss = w.stride(3);
  auto out = at::empty(src.sizes(), src.options().memory_format(
                                       at::MemoryFormat::ChannelsLast));
  if (src.scalar_type() == at::kHalf)
    launch_dwk<_Float16, DGRAD>(src, w, out, d, (int)w.size(2));
  else
    launch_dwk<__bf16, DGRAD>(src, w, out, d, (int)w.size(2));
  return out;
}

template <typename T, int K>
void launch_wgrad_k(const at::Tensor& dy, const at::Tensor& x,
                    at::Tensor& slab, at::Tensor& dw, const DwkDims& d,
                    int splits) {
  const dim3 grid(splits, (d.C + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL((conv_dwk_wgrad_kernel<T, K>), grid, dim3(256), 0,
                     dwk_stream(), reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     slab.data_ptr<float>(), d);
  const int rblocks = (int)std::min((K * K * (long)d.C + 255) / 256, 2048L);
  hipLaunchKernelGGL(dwk_wgrad_reduce_kernel<T>, dim3(rblocks), dim3(256), 0,
                     dwk_stream(), slab.data_ptr<float>(),
                     reinterpret_cast<T*>(dw.data_ptr()), d.C, K * K, splits);
}

template <typename T>
void launch_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& slab,
                  at::Tensor& dw, const DwkDims& d, int K, int splits) {
  if (K == 5) launch_wgrad_k<T, 5>(dy, x, slab, dw, d, splits);
  else if (K == 7) launch_wgrad_k<T, 7>(dy, x, slab, dw, d, splits);
  else launch_wgrad_k<T, 9>(dy, x, slab, dw, d, splits);
}

}  // namespace

at::Tensor conv_dwk_fwd(at::Tensor x, at::Tensor w) {
  return run_dwk<false>(x, "x", w);
}

// stride 1: dx has dy's extents
at::Tensor conv_dwk_dgrad(at::Tensor dy, at::Tensor w) {
  return run_dwk<true>(dy, "dy", w);
}

// splits: 0 = about four blocks per CU over all chunks, at most one per work
// item; a positive count is taken as it is (blocks past the work write zeros).
at::Tensor conv_dwk_wgrad(at::Tensor dy, at::Tensor x, long K, long splits) {
  check_act(dy, "dy");
  check_act(x, "x");
  check_same_16(dy, "dy", x, "x");
  check_k(K);
  TORCH_CHECK(dy.sizes() == x.sizes(), "depthwise KxK conv: dy ", dy.sizes(),
              " and x ", x.sizes(), " must have the same extents");
  TORCH_CHECK(splits >= 0 && splits <= 65535,
              "depthwise KxK conv: splits must be in 0..65535, got ", splits);
  const DwkDims d = make_dims(x);
  const long C = d.C;
  const long work = (long)d.N * d.tiles_h * d.tiles_w;
  const long chunks = (C + CHUNK - 1) / CHUNK;
  if (splits == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    splits = std::min(std::max(1L, 4 * cus / chunks), std::min(work, 65535L));
  }
  auto slab = at::empty({splits, K * K, C}, x.options().dtype(at::kFloat));
  auto dw = at::empty({C, 1, K, K}, x.options().memory_format(
                                        at::MemoryFormat::Contiguous));
  if (x.scalar_type() == at::kHalf)
    launch_wgrad<_Float16>(dy, x, slab, dw, d, (int)K, (int)splits);
  else
    launch_wgrad<__bf16>(dy, x, slab, dw, d, (int)K, (int)splits);
  return dw;
}
