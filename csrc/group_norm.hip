// MI355X (gfx950/CDNA4) Group Normalization (Wu & He 2018) joined with the
// residual add and ReLU:
//   y = act((x - mean[n, g]) * rstd[n, g] * gamma[c] + beta[c] (+ residual))
// x, residual, y: NHWC bf16 or fp16, C a multiple of 8, G groups of Cg = C / G
// channels, Cg in {2, 4, 8, 16, 32, 64}. gamma, beta, mean [N, G], rstd [N, G]
// and every sum are fp32; a result is rounded once and stored 16 bytes wide.
//
// The statistics of a group are per image, so one block owns a complete
// reduction domain and there is no partials pass: the forward is ONE launch,
// the backward one launch and a small reduce for dgamma and dbeta.
//
// Work split (the lane geometry of conv_depthwise.hip and se_block.hip). A
// block of 256 threads owns one image and a chunk of CW channels, CW = 64 or
// 32: tid % (CW / 8) is a lane's 8 consecutive channels, tid / (CW / 8) one
// of 32 (CW = 64) or 64 (CW = 32) pixel slots striding over HW. Cg divides
// CW, so a chunk holds whole groups; the last chunk may be ragged and is
// predicated on c < C. grid (N, ceil(C / CW)).
//
// LDS residency. gfx950 has 160 KB of LDS; the block keeps its [CAP][CW] slice
// of x in a static tile, CAP the smallest capacity >= HW, so x is read from
// HBM once and y written once, and the statistics are two-pass (mean, then
// centred squares out of LDS; never E[x^2] - mean^2). A lane reads back only
// what it wrote itself. A layer with more pixels than the largest capacity
// runs the CAP = 0 instantiation, which walks global memory again instead.
// Both walk the pixels and fold the sums in the same order, so for one CW
// they give the same bits; MI355X_GN_RESIDENT=0 selects CAP = 0 everywhere.
//
// Sum order. A lane sums its pixels in ascending order, four 16-byte loads
// per operand in flight at a time (a 128 KB block leaves four waves on the
// CU); the slots are folded through an 8 KB scratch in slot order, then the
// channels of a group in channel order. No atomics anywhere.
//
// gn_fwd_kernel<T, CW = 64, CAP in {0, 64, 256, 1024}>
//   pass A  x -> tile, channel sums -> mean[g]
//   pass B  sum (x - mean)^2 -> rstd[g] = 1 / sqrt(var + eps)
//   pass C  y, with the residual read once from global memory
// gn_bwd_kernel<T, CW, CAP>, g = dy * (y > 0) under ReLU, else dy
//   pass A  reads dy, y, x; keeps g and x in two tiles; per channel
//           a[c] = sum g, b[c] = sum g * xhat: row n of the fp32 slab
//           [N][2][C], and s1[g] = sum_c gamma a, s2[g] = sum_c gamma b
//   pass B  dx = rstd * (g * gamma - (s1 + xhat * s2) / (Cg * HW)), and
//           d_residual = g when a residual was given
//   two tiles: CW = 64 with CAP in {64, 256, 576}; CW = 32 with CAP = 1152
//   while HW <= 1152 and Cg <= 32; else CAP = 0 (reads dy, y, x twice).
//   The largest tile set is 144 KB, 153 KB with the scratch: under the
//   163840-byte limit of a block.
// gn_param_grad_reduce_kernel
//   sums the slab over n in image order: a block takes 32 columns of [2][C]
//   and 8 slices of the batch, folded through LDS in slice order.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>

#include <cstdlib>
#include <cstring>
#include <tuple>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int UNROLL = 4;    // pixels of a lane whose loads are in flight
constexpr int FOLD = 2048;   // floats of the slot scratch: slots * CW
constexpr int RC = 32;       // columns per reduce block
constexpr int RS = 8;        // batch slices per reduce block

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

__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
  const f32x4 a = reinterpret_cast<const f32x4*>(p)[0];
  const f32x4 b = reinterpret_cast<const f32x4*>(p)[1];
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
  f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

// A lane's pixels slot, slot + SLOTS, ... < HW in ascending order: load(p, v)
// of UNROLL pixels are issued before their use(p, v). v is NV vectors.
template <int SLOTS, int NV, typename Load, typename Use>
__device__ __forceinline__ void walk(int HW, int slot, Load load, Use use) {
  for (int p0 = slot; p0 < HW; p0 += UNROLL * SLOTS) {
    u32x4 v[UNROLL][NV];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j)
      if (p0 + j * SLOTS < HW) load(p0 + j * SLOTS, v[j]);
#pragma unroll
    for (int j = 0; j < UNROLL; ++j)
      if (p0 + j * SLOTS < HW) use(p0 + j * SLOTS, v[j]);
  }
}

// chs[c] = the block's sum of acc for channel c of the chunk: the slots in
// slot order. Opens with a barrier, so `fold` and `chs` may have readers.
template <int CW>
__device__ __forceinline__ void fold_slots(const float (&acc)[8], float* fold,
                                           float* chs) {
  constexpr int LPC = CW / 8, SLOTS = 256 / LPC;
  static_assert(SLOTS * CW == FOLD, "the scratch is slots x channels");
  const int cl = threadIdx.x % LPC, slot = threadIdx.x / LPC;
  __syncthreads();
  f32x4* fd = reinterpret_cast<f32x4*>(fold + slot * CW + cl * 8);
  fd[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  fd[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  __syncthreads();
  if (threadIdx.x < CW) {
    float s = 0.f;
#pragma unroll 8
    for (int sl = 0; sl < SLOTS; ++sl) s += fold[sl * CW + threadIdx.x];
    chs[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int CW, int CAP>
__global__ __launch_bounds__(256)
void gn_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                   const float* __restrict__ gamma,
                   const float* __restrict__ beta, T* __restrict__ y,
                   float* __restrict__ mean, float* __restrict__ rstd, int C,
                   int HW, int G, int cg_shift, float eps, int relu) {
  constexpr int LPC = CW / 8, SLOTS = 256 / LPC;
  __shared__ u32x4 tile[CAP > 0 ? CAP * LPC : 1];
  __shared__ float fold[FOLD];
  __shared__ float chs[CW];
  __shared__ float gstat[CW / 2];   // Cg >= 2
  const int cl = threadIdx.x % LPC, slot = threadIdx.x / LPC;
  const int n = blockIdx.x, c0 = blockIdx.y * CW, ch = c0 + cl * 8;
  const bool live = ch < C;         // C % 8 == 0: a lane is whole or empty
  const int hw = live ? HW : 0;     // an empty lane walks nothing, sums zeros
  const int Cg = 1 << cg_shift, groups = CW >> cg_shift;
  const float count = (float)Cg * (float)HW;
  const size_t base = ((size_t)n * HW * C + (live ? ch : 0)) >> 3;
  const size_t C8 = (size_t)(C >> 3);
  const u32x4* xv = reinterpret_cast<const u32x4*>(x) + base;

  // pass A: channel sums; the tile is filled
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  walk<SLOTS, 1>(hw, slot,
      [&](int p, u32x4 (&v)[1]) { v[0] = xv[p * C8]; },
      [&](int p, u32x4 (&v)[1]) {
        if constexpr (CAP > 0) tile[p * LPC + cl] = v[0];
        float a[8];
        unpack8<T>(v[0], a);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += a[i];
      });
  fold_slots<CW>(acc, fold, chs);
  if (threadIdx.x < groups) {       // the channels of a group, in order
    float s = 0.f;
    for (int i = 0; i < Cg; ++i) s += chs[threadIdx.x * Cg + i];
    gstat[threadIdx.x] = s / count;
  }
  __syncthreads();
  float m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = gstat[(cl * 8 + i) >> cg_shift];
  const int gl = (c0 >> cg_shift) + threadIdx.x;
  if (threadIdx.x < groups && gl < G)
    mean[(size_t)n * G + gl] = gstat[threadIdx.x];

  // pass B: centred squares, out of the tile when there is one
  auto load_x = [&](int p, u32x4* v) {
    if constexpr (CAP > 0) v[0] = tile[p * LPC + cl];
    else v[0] = xv[p * C8];
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  walk<SLOTS, 1>(hw, slot,
      [&](int p, u32x4 (&v)[1]) { load_x(p, v); },
      [&](int, u32x4 (&v)[1]) {
        float a[8];
        unpack8<T>(v[0], a);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = a[i] - m[i];
          acc[i] = fmaf(d, d, acc[i]);
        }
      });
  fold_slots<CW>(acc, fold, chs);   // its first barrier: gstat has been read
  if (threadIdx.x < groups) {
    float s = 0.f;
    for (int i = 0; i < Cg; ++i) s += chs[threadIdx.x * Cg + i];
    const float r = 1.f / sqrtf(s / count + eps);
    gstat[threadIdx.x] = r;
    if (gl < G) rstd[(size_t)n * G + gl] = r;
  }
  __syncthreads();
  if (!live) return;                // no barrier follows

  // pass C: normalize, affine, add, ReLU; one rounding
  float r[8], ga[8], be[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = gstat[(cl * 8 + i) >> cg_shift];
  load8(gamma + ch, ga);
  load8(beta + ch, be);
  const u32x4* rv = reinterpret_cast<const u32x4*>(res) + base;
  u32x4* yv = reinterpret_cast<u32x4*>(y) + base;
  walk<SLOTS, 2>(hw, slot,
      [&](int p, u32x4 (&v)[2]) {
        load_x(p, v);
        if (res) v[1] = rv[p * C8];
      },
      [&](int p, u32x4 (&v)[2]) {
        float a[8], b[8];
        unpack8<T>(v[0], a);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          a[i] = fmaf((a[i] - m[i]) * r[i], ga[i], be[i]);
        if (res) {
          unpack8<T>(v[1], b);
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] += b[i];
        }
        if (relu) {
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = fmaxf(a[i], 0.f);
        }
        yv[p * C8] = pack8<T>(a);
      });
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <typename T, int CW, int CAP>
__global__ __launch_bounds__(256)
void gn_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                   const T* __restrict__ x, const float* __restrict__ mean,
                   const float* __restrict__ rstd,
                   const float* __restrict__ gamma, T* __restrict__ dx,
                   T* __restrict__ dres, float* __restrict__ slab, int C,
                   int HW, int G, int cg_shift, int relu) {
  constexpr int LPC = CW / 8, SLOTS = 256 / LPC;
  __shared__ u32x4 tile_g[CAP > 0 ? CAP * LPC : 1];
  __shared__ u32x4 tile_x[CAP > 0 ? CAP * LPC : 1];
  __shared__ float fold[FOLD];
  __shared__ float cha[CW], chb[CW];
  __shared__ float gs1[CW / 2], gs2[CW / 2];
  const int cl = threadIdx.x % LPC, slot = threadIdx.x / LPC;
  const int n = blockIdx.x, c0 = blockIdx.y * CW, ch = c0 + cl * 8;
  const bool live = ch < C;
  const int hw = live ? HW : 0;
  const int Cg = 1 << cg_shift, groups = CW >> cg_shift;
  const float count = (float)Cg * (float)HW;
  const size_t base = ((size_t)n * HW * C + (live ? ch : 0)) >> 3;
  const size_t C8 = (size_t)(C >> 3);
  const u32x4* dyv = reinterpret_cast<const u32x4*>(dy) + base;
  const u32x4* yv = reinterpret_cast<const u32x4*>(y) + base;
  const u32x4* xv = reinterpret_cast<const u32x4*>(x) + base;

  float m[8], r[8], ga[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = r[i] = ga[i] = 0.f;
  if (live) {                       // whole groups: ch + i < C is group < G
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const size_t at = (size_t)n * G + ((ch + i) >> cg_shift);
      m[i] = mean[at];
      r[i] = rstd[at];
    }
    load8(gamma + ch, ga);
  }

  // v -> g = dy * (y > 0) or dy, and x; the same values in both passes
  auto load_gx = [&](int p, u32x4* v) {
    v[0] = dyv[p * C8];
    v[1] = xv[p * C8];
    if (relu) v[2] = yv[p * C8];
  };
  auto form_g = [&](u32x4* v, float (&g)[8]) {
    unpack8<T>(v[0], g);
    if (relu) {
      float o[8];
      unpack8<T>(v[2], o);
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = o[i] > 0.f ? g[i] : 0.f;
    }
  };

  // pass A: a[c] = sum g, b[c] = sum g * xhat; the tiles are filled
  float a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = b[i] = 0.f;
  walk<SLOTS, 3>(hw, slot,
      [&](int p, u32x4 (&v)[3]) { load_gx(p, v); },
      [&](int p, u32x4 (&v)[3]) {
        float g[8], xx[8];
        form_g(v, g);
        unpack8<T>(v[1], xx);
        if constexpr (CAP > 0) {    // g is dy or zero: packing it is exact
          tile_g[p * LPC + cl] = pack8<T>(g);
          tile_x[p * LPC + cl] = v[1];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          a[i] += g[i];
          b[i] = fmaf(g[i], (xx[i] - m[i]) * r[i], b[i]);
        }
      });
  fold_slots<CW>(a, fold, cha);
  fold_slots<CW>(b, fold, chb);
  if (threadIdx.x < CW && c0 + threadIdx.x < C) {
    float* row = slab + (size_t)n * 2 * C + c0 + threadIdx.x;
    row[0] = cha[threadIdx.x];      // this image's share of dbeta
    row[C] = chb[threadIdx.x];      //                    and of dgamma
  }
  if (threadIdx.x < groups && c0 + threadIdx.x * Cg < C) {
    float s1 = 0.f, s2 = 0.f;       // the channels of a group, in order
    for (int i = 0; i < Cg; ++i) {
      const int cc = threadIdx.x * Cg + i;
      const float gm = gamma[c0 + cc];
      s1 = fmaf(gm, cha[cc], s1);
      s2 = fmaf(gm, chb[cc], s2);
    }
    gs1[threadIdx.x] = s1 / count;
    gs2[threadIdx.x] = s2 / count;
  }
  __syncthreads();
  if (!live) return;                // no barrier follows

  // pass B: dx, and d_residual = g
  float s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s1[i] = gs1[(cl * 8 + i) >> cg_shift];
    s2[i] = gs2[(cl * 8 + i) >> cg_shift];
  }
  u32x4* dxv = reinterpret_cast<u32x4*>(dx) + base;
  u32x4* drv = reinterpret_cast<u32x4*>(dres) + base;
  walk<SLOTS, 3>(hw, slot,
      [&](int p, u32x4 (&v)[3]) {
        if constexpr (CAP > 0) {
          v[0] = tile_g[p * LPC + cl];
          v[1] = tile_x[p * LPC + cl];
        } else {
          load_gx(p, v);
        }
      },
      [&](int p, u32x4 (&v)[3]) {
        float g[8], xx[8];
        if constexpr (CAP > 0) unpack8<T>(v[0], g);
        else form_g(v, g);
        unpack8<T>(v[1], xx);
        if (dres) drv[p * C8] = pack8<T>(g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xx[i] - m[i]) * r[i];
          xx[i] = r[i] * (g[i] * ga[i] - fmaf(xh, s2[i], s1[i]));
        }
        dxv[p * C8] = pack8<T>(xx);
      });
}

// out[j] = sum_n slab[n][j], j < cols = 2 C, in image order: slice s of a
// block sums images [s * per, (s + 1) * per), then the slices fold in order.
__global__ __launch_bounds__(RC * RS)
void gn_param_grad_reduce_kernel(const float* __restrict__ slab,
                                 float* __restrict__ out, int N, int cols,
                                 int per) {
  __shared__ float f[RS][RC];
  const int cc = threadIdx.x % RC, s = threadIdx.x / RC;
  const int j = blockIdx.x * RC + cc;
  float acc = 0.f;
  if (j < cols) {
    const int n1 = min(N, (s + 1) * per);
#pragma unroll 4
    for (int n = s * per; n < n1; ++n) acc += slab[(size_t)n * cols + j];
  }
  f[s][cc] = acc;
  __syncthreads();
  if (s == 0 && j < cols) {
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < RS; ++t) sum += f[t][cc];
    out[j] = sum;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
hipStream_t gn_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline bool resident_wanted() {
  const char* e = std::getenv("MI355X_GN_RESIDENT");
  return !(e && std::strcmp(e, "0") == 0);
}

inline void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 ||
                              t.scalar_type() == at::kHalf),
              "group norm: ", name, " must be a bf16 or fp16 HIP tensor, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.numel() > 0 &&
              t.is_contiguous(at::MemoryFormat::ChannelsLast),
              "group norm: ", name, " must be 4-D channels_last");
  TORCH_CHECK(t.size(1) % 8 == 0, "group norm: C must be a multiple of 8, "
              "got ", t.size(1));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "group norm: ", name, " must be 16-byte aligned");
  TORCH_CHECK(t.numel() / 8 < (1L << 31) && t.size(1) < (1L << 22) &&
              t.size(2) * t.size(3) < (1L << 28),
              "group norm: ", name, " is too large (2^34 elements, 2^22 "
              "channels or 2^28 pixels)");
}

inline void check_like(const at::Tensor& t, const char* name,
                       const at::Tensor& x) {
  check_act(t, name);
  TORCH_CHECK(t.scalar_type() == x.scalar_type() && t.sizes() == x.sizes(),
              "group norm: ", name, " must have the dtype and shape of x, "
              "got ", t.scalar_type(), " ", t.sizes(), " for ",
              x.scalar_type(), " ", x.sizes());
}

inline void check_f32(const at::Tensor& t, const char* name,
                      at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
              t.is_contiguous(),
              "group norm: ", name, " must be a contiguous fp32 HIP tensor, "
              "got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, "group norm: ", name, " must be ", shape,
              ", got ", t.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "group norm: ", name, " must be 16-byte aligned");
}

// log2 of the channels per group
inline int check_groups(long C, long groups) {
  TORCH_CHECK(groups >= 1 && C % groups == 0,
              "group norm: groups must divide C, got ", groups, " for C = ", C);
  const long Cg = C / groups;
  TORCH_CHECK(Cg == 2 || Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 ||
              Cg == 64,
              "group norm: channels per group must be 2, 4, 8, 16, 32 or 64, "
              "got ", Cg);
  return __builtin_ctzl((unsigned long)Cg);
}

template <typename T>
void launch_fwd(const at::Tensor& x, const at::Tensor* res,
                const at::Tensor& gamma, const at::Tensor& beta, at::Tensor& y,
                at::Tensor& mean, at::Tensor& rstd, int G, int cg_shift,
                float eps, bool relu) {
  const int N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  const int cap = !resident_wanted() || HW > 1024 ? 0
                  : HW <= 64 ? 64 : HW <= 256 ? 256 : 1024;
  const dim3 grid(N, (C + 63) / 64);
#define GN_FWD(CAP)                                                          \
  hipLaunchKernelGGL((gn_fwd_kernel<T, 64, CAP>), grid, dim3(256), 0,        \
                     gn_stream(), reinterpret_cast<const T*>(x.data_ptr()),  \
                     res ? reinterpret_cast<const T*>(res->data_ptr())       \
                         : nullptr,                                          \
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),        \
                     reinterpret_cast<T*>(y.data_ptr()),                     \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), C, HW,  \
                     G, cg_shift, eps, (int)relu)
  if (cap == 0) GN_FWD(0);
  else if (cap == 64) GN_FWD(64);
  else if (cap == 256) GN_FWD(256);
  else GN_FWD(1024);
#undef GN_FWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <typename T>
void launch_bwd(const at::Tensor& dy, const at::Tensor& y, const at::Tensor& x,
                const at::Tensor& mean, const at::Tensor& rstd,
                const at::Tensor& gamma, at::Tensor& dx, at::Tensor* dres,
                at::Tensor& slab, int G, int cg_shift, bool relu) {
  const int N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  // two tiles: 64 channels up to 576 px, 32 channels up to 1152 px
  const int cw = HW <= 576 ? 64 : HW <= 1152 && cg_shift <= 5 ? 32 : 64;
  const int cap = !resident_wanted() || HW > 1152 ? 0
                  : cw == 32 ? 1152
                  : HW <= 64 ? 64 : HW <= 256 ? 256 : HW <= 576 ? 576 : 0;
  const dim3 grid(N, (C + cw - 1) / cw);
#define GN_BWD(CW, CAP)                                                      \
  hipLaunchKernelGGL((gn_bwd_kernel<T, CW, CAP>), grid, dim3(256), 0,        \
                     gn_stream(), reinterpret_cast<const T*>(dy.data_ptr()), \
                     reinterpret_cast<const T*>(y.data_ptr()),               \
                     reinterpret_cast<const T*>(x.data_ptr()),               \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                     gamma.data_ptr<float>(),                                \
                     reinterpret_cast<T*>(dx.data_ptr()),                    \
                     dres ? reinterpret_cast<T*>(dres->data_ptr()) : nullptr,\
                     slab.data_ptr<float>(), C, HW, G, cg_shift, (int)relu)
  if (cw == 32) { if (cap == 0) GN_BWD(32, 0); else GN_BWD(32, 1152); }
  else if (cap == 0) GN_BWD(64, 0);
  else if (cap == 64) GN_BWD(64, 64);
  else if (cap == 256) GN_BWD(64, 256);
  else GN_BWD(64, 576);
#undef GN_BWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace

// -> (y, mean [N, G], rstd [N, G])
std::tuple<at::Tensor, at::Tensor, at::Tensor> gn_fwd(
    at::Tensor x, at::Tensor gamma, at::Tensor beta,
    c10::optional<at::Tensor> residual, long groups, double eps, bool relu) {
  check_act(x, "x");
  const long N = x.size(0), C = x.size(1);
  const int cg_shift = check_groups(C, groups);
  check_f32(gamma, "gamma", {C});
  check_f32(beta, "beta", {C});
  const at::Tensor* res = nullptr;
  if (residual.has_value() && residual->defined()) {
    check_like(*residual, "residual", x);
    res = &*residual;
  }
  auto y = at::empty_like(x);
  auto mean = at::empty({N, groups}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N, groups}, x.options().dtype(at::kFloat));
  if (x.scalar_type() == at::kHalf)
    launch_fwd<_Float16>(x, res, gamma, beta, y, mean, rstd, (int)groups,
                         cg_shift, (float)eps, relu);
  else
    launch_fwd<__bf16>(x, res, gamma, beta, y, mean, rstd, (int)groups,
                       cg_shift, (float)eps, relu);
  return {y, mean, rstd};
}

// -> (dx, d_residual or an undefined tensor, dgamma [C], dbeta [C]); with
// `relu`, y is the forward's result and masks dy
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> gn_bwd(
    at::Tensor dy, at::Tensor y, at::Tensor x, at::Tensor mean,
    at::Tensor rstd, at::Tensor gamma, long groups, bool relu,
    bool has_residual) {
  check_act(x, "x");
  check_like(dy, "dy", x);
  check_like(y, "y", x);
  const long N = x.size(0), C = x.size(1);
  const int cg_shift = check_groups(C, groups);
  check_f32(mean, "mean", {N, groups});
  check_f32(rstd, "rstd", {N, groups});
  check_f32(gamma, "gamma", {C});
  auto dx = at::empty_like(x);
  at::Tensor dres;
  if (has_residual) dres = at::empty_like(x);
  auto slab = at::empty({N, 2, C}, x.options().dtype(at::kFloat));
  auto grads = at::empty({2, C}, x.options().dtype(at::kFloat));
  if (x.scalar_type() == at::kHalf)
    launch_bwd<_Float16>(dy, y, x, mean, rstd, gamma, dx,
                         has_residual ? &dres : nullptr, slab, (int)groups,
                         cg_shift, relu);
  else
    launch_bwd<__bf16>(dy, y, x, mean, rstd, gamma, dx,
                       has_residual ? &dres : nullptr, slab, (int)groups,
                       cg_shift, relu);
  const int cols = (int)(2 * C), per = (int)((N + RS - 1) / RS);
  hipLaunchKernelGGL(gn_param_grad_reduce_kernel, dim3((cols + RC - 1) / RC),
                     dim3(RC * RS), 0, gn_stream(), slab.data_ptr<float>(),
                     grads.data_ptr<float>(), (int)N, cols, per);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dres, grads[1], grads[0]};
}
