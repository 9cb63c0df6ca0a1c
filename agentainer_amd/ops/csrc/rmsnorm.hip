// RMSNorm kernels (gfx950) — memory-bound, bf16x8 vectorized.
//
// Serves the Llama/Mixtral forward of the agent engine (SURVEY.md §2.3
// "RMSNorm kernel" row; reference has no GPU code — this is new work).
//
// Three entry points:
//   rmsnorm(out, x, w, eps):            out = x * rsqrt(mean(x^2)+eps) * w
//   fused_add_rmsnorm(out, x, res, w):  res += x;  out = rmsnorm(res)
//   splitk_add_rmsnorm(out, ws, S, ..): res += bf16(sum_s ws[s]); out = rmsnorm(res)
//
// Design notes (cdna_hip_programming.md G13): hipcc does not vectorize
// scalar bf16 loads — all global access is 16 B/lane (bf16x8). One
// workgroup (256 threads) per row; f32 accumulation; wave shuffle + LDS
// cross-wave reduction. Hidden sizes up to 16384 handled by grid-stride
// over 2048-element chunks.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

// Shared tail of the single-pass kernels: block-wide sum of squares, then
// scale the register-resident row by rms * w and store it.
template <int VPT>
__device__ __forceinline__ void rms_scale_store(
    short* __restrict__ out, const short* __restrict__ w,
    const bf16x8 (&v)[VPT], float ss, long base, int H, float eps) {
  __shared__ float red[8];
  const int tid = threadIdx.x;
  ss = wave_sum(ss);
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = ss;
  __syncthreads();
  ss = 0.f;
#pragma unroll
  for (int wv = 0; wv < 8; ++wv) ss += red[wv];
  const float rms = rsqrtf(ss / (float)H + eps);

#pragma unroll
  for (int r = 0; r < VPT; ++r) {
    const int i = (tid + r * 512) * 8;
    if (i < H) {
      bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + i);
      bf16x8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ov[j] = f2bits(bits2f(v[r][j]) * rms * bits2f(wv[j]));
      *reinterpret_cast<bf16x8*>(out + base + i) = ov;
    }
  }
}

// Single-pass: the row lives in registers between the reduction and the
// scale, so x (and the fused residual sum) is read from HBM exactly once.
// 512 threads/block; VPT = ceil(H / 4096) bf16x8 vectors per thread.
template <bool FUSED_ADD, int VPT>
__global__ __launch_bounds__(512) void rmsnorm_kernel(
    short* __restrict__ out, const short* __restrict__ x,
    short* __restrict__ residual, const short* __restrict__ w, float eps,
    int H) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const long base = (long)row * H;

  bf16x8 v[VPT];
  float ss = 0.f;
#pragma unroll
  for (int r = 0; r < VPT; ++r) {
    const int i = (tid + r * 512) * 8;
    if (i < H) {
      v[r] = *reinterpret_cast<const bf16x8*>(x + base + i);
      if (FUSED_ADD) {
        bf16x8 rv = *reinterpret_cast<const bf16x8*>(residual + base + i);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[r][j] = f2bits(bits2f(v[r][j]) + bits2f(rv[j]));
        *reinterpret_cast<bf16x8*>(residual + base + i) = v[r];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bits2f(v[r][j]);
        ss = fmaf(f, f, ss);
      }
    } else {
      v[r] = bf16x8{};
    }
  }
  rms_scale_store<VPT>(out, w, v, ss, base, H, eps);
}

// fused_add_rmsnorm whose x is still the skinny GEMM's split-K partials
// ws[S][M][H] (f32): x = bf16(sum_s ws[s]) is formed in registers, in the
// slab order and with the rounding of splitk_combine_kernel, so out and
// residual are bit-identical to combine -> rmsnorm_kernel<true> while the
// combine launch and its bf16 round trip through memory are gone.
// S_CT > 0: compile-time slab count, every slab load issued before the
// first add (the 64-block grid is latency-bound, not bandwidth-bound);
// S_CT == 0: runtime S. Loads use a clamped column instead of a per-lane
// branch; lanes past H only skip the stores.
template <int VPT, int S_CT>
__global__ __launch_bounds__(512) void splitk_add_rmsnorm_kernel(
    short* __restrict__ out, const float* __restrict__ ws,
    short* __restrict__ residual, const short* __restrict__ w, float eps,
    int H, int S, long slab) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const long base = (long)row * H;

  bf16x8 v[VPT];
  float ss = 0.f;
#pragma unroll
  for (int r = 0; r < VPT; ++r) {
    const int i = (tid + r * 512) * 8;
    const bool alive = i < H;
    const long off = base + (alive ? i : 0);
    const float* p = ws + off;
    f32x4 lo, hi;
    if constexpr (S_CT > 0) {
      f32x4 pl[S_CT], ph[S_CT];
#pragma unroll
      for (int s = 0; s < S_CT; ++s) {
        pl[s] = *reinterpret_cast<const f32x4*>(p + s * slab);
        ph[s] = *reinterpret_cast<const f32x4*>(p + s * slab + 4);
      }
      lo = pl[0];
      hi = ph[0];
#pragma unroll
      for (int s = 1; s < S_CT; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lo[j] += pl[s][j];
          hi[j] += ph[s][j];
        }
      }
    } else {
      lo = *reinterpret_cast<const f32x4*>(p);
      hi = *reinterpret_cast<const f32x4*>(p + 4);
      for (int s = 1; s < S; ++s) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + s * slab);
        const f32x4 b = *reinterpret_cast<const f32x4*>(p + s * slab + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lo[j] += a[j];
          hi[j] += b[j];
        }
      }
    }
    const bf16x8 rv = *reinterpret_cast<const bf16x8*>(residual + off);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const short xb = f2bits(j < 4 ? lo[j & 3] : hi[j & 3]);
      v[r][j] = f2bits(bits2f(xb) + bits2f(rv[j]));
    }
    if (alive) {
      *reinterpret_cast<bf16x8*>(residual + off) = v[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bits2f(v[r][j]);
        ss = fmaf(f, f, ss);
      }
    } else {
      v[r] = bf16x8{};
    }
  }
  rms_scale_store<VPT>(out, w, v, ss, base, H, eps);
}

}  // namespace

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor w, double eps) {
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "rmsnorm: bf16 only");
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
  const int T = x.numel() / H;
  auto stream = at::hip::getCurrentHIPStream();
#define RN_LAUNCH(VPT)                                                         \
  hipLaunchKernelGGL((rmsnorm_kernel<false, VPT>), dim3(T), dim3(512), 0,      \
                     stream, (short*)out.data_ptr(),                           \
                     (const short*)x.data_ptr(), nullptr,                      \
                     (const short*)w.data_ptr(), (float)eps, H)
  if (H <= 4096) RN_LAUNCH(1);
  else if (H <= 8192) RN_LAUNCH(2);
  else if (H <= 16384) RN_LAUNCH(4);
  else TORCH_CHECK(false, "rmsnorm: hidden > 16384 unsupported");
#undef RN_LAUNCH
}

void fused_add_rmsnorm(torch::Tensor out, torch::Tensor x,
                       torch::Tensor residual, torch::Tensor w, double eps) {
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && w.is_contiguous() &&
              residual.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fused_add_rmsnorm: bf16 only");
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
  const int T = x.numel() / H;
  auto stream = at::hip::getCurrentHIPStream();
#define RNF_LAUNCH(VPT)                                                        \
  hipLaunchKernelGGL((rmsnorm_kernel<true, VPT>), dim3(T), dim3(512), 0,       \
                     stream, (short*)out.data_ptr(),                           \
                     (const short*)x.data_ptr(), (short*)residual.data_ptr(),  \
                     (const short*)w.data_ptr(), (float)eps, H)
  if (H <= 4096) RNF_LAUNCH(1);
  else if (H <= 8192) RNF_LAUNCH(2);
  else if (H <= 16384) RNF_LAUNCH(4);
  else TORCH_CHECK(false, "rmsnorm: hidden > 16384 unsupported");
#undef RNF_LAUNCH
}

void splitk_add_rmsnorm(torch::Tensor out, torch::Tensor ws, long split,
                        long M, long N, torch::Tensor residual,
                        torch::Tensor w, double eps) {
  TORCH_CHECK(out.is_contiguous() && ws.is_contiguous() &&
              residual.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(ws.scalar_type() == at::kFloat,
              "splitk_add_rmsnorm: f32 partials");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 &&
                  residual.scalar_type() == at::kBFloat16 &&
                  w.scalar_type() == at::kBFloat16,
              "splitk_add_rmsnorm: bf16 only");
  const int H = residual.size(-1);
  TORCH_CHECK(N == H, "splitk_add_rmsnorm: GEMM N must equal the hidden size");
  TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
  TORCH_CHECK(M >= 1 && residual.numel() == M * N && out.numel() == M * N &&
                  w.numel() == H,
              "splitk_add_rmsnorm: shape mismatch");
  TORCH_CHECK(split >= 1 && ws.numel() >= split * M * N,
              "splitk_add_rmsnorm: split-K workspace too small");
  auto stream = at::hip::getCurrentHIPStream();
#define SKN_LAUNCH(VPT, S_CT)                                                  \
  hipLaunchKernelGGL((splitk_add_rmsnorm_kernel<VPT, S_CT>), dim3((int)M),     \
                     dim3(512), 0, stream, (short*)out.data_ptr(),             \
                     ws.data_ptr<float>(), (short*)residual.data_ptr(),        \
                     (const short*)w.data_ptr(), (float)eps, H, (int)split,    \
                     (long)(M * N))
#define SKN_SPLIT(VPT)                                                         \
  do {                                                                         \
    if (split == 4) SKN_LAUNCH(VPT, 4);                                        \
    else if (split == 8) SKN_LAUNCH(VPT, 8);                                   \
    else SKN_LAUNCH(VPT, 0);                                                   \
  } while (0)
  if (H <= 4096) SKN_SPLIT(1);
  else if (H <= 8192) SKN_SPLIT(2);
  else if (H <= 16384) SKN_SPLIT(4);
  else TORCH_CHECK(false, "rmsnorm: hidden > 16384 unsupported");
#undef SKN_SPLIT
#undef SKN_LAUNCH
}
