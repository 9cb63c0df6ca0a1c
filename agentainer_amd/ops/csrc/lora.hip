// Batched multi-LoRA decode kernels (gfx950) — "BGMV": every token row
// picks its own adapter by a device-resident index.
//
// Serves per-agent LoRA adapters on a shared base model: the decode step
// is hipGraph-captured, so which adapter a row uses has to be data read
// inside the captured body (ids[t]), never a host loop over adapters.
//
// Two entry points, applied after a base projection GEMM wrote y:
//   lora_shrink(v, x, A, ids):      v[t, r]  = sum_k A[ids[t], r, k] * x[t, k]
//   lora_expand_add(y, v, B, ids):  y[t, n] += sum_r B[ids[t], n, r] * v[t, r]
// x bf16 [T, K] (row stride), A bf16 [S, R, K], v f32 [T, R],
// y bf16 [T, N] (row stride), B bf16 [S, N, R], ids int32 [T].
// v stays f32 between the two (no bf16 round trip of the rank-space
// vector); the adapter scale alpha/r is folded into B when it is loaded.
//
// ids[t] < 0 marks a base-model row and is also what graph pad rows
// carry: shrink writes zeros to v[t, :] without reading A, expand-add
// neither loads nor stores y[t, :], so such rows stay bit-identical.
// 0 <= ids[t] < S is the caller's contract; an id >= S is treated like a
// negative one, so a bad id can never read outside the pool.
//
// Design notes (decode: T <= 256, R <= 64, a handful of adapters whose
// A/B are a few hundred KB per projection and sit in L2 / Infinity Cache
// after the first row touches them — both kernels are latency- and
// launch-bound, not HBM-bound, and rows share no operand, so no MFMA):
//   * all global access to x, A, B and y is 16 B/lane (bf16x8; G13:
//     hipcc does not vectorize scalar bf16 loads);
//   * shrink: grid (T, R/8), 4 waves per block, each wave owns TWO rank
//     rows so one x vector feeds two A vectors; lanes stride K by
//     64*8 elements, f32 fmaf accumulation, wave_sum, lane 0 stores;
//   * expand-add: grid (T, ceil(N/8/256)); the row's v goes to LDS once
//     per block and from there into registers (compile-time R/8 for the
//     pool ranks 8/16/32/48, a runtime loop otherwise); each thread owns
//     8 whole output columns = one 16-B y vector, and walks the 8 B rows
//     of those columns (8*R contiguous bf16) with 16-B loads.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int SHRINK_WAVES = 4;
constexpr int SHRINK_RPW = 2;  // rank rows per wave
constexpr int SHRINK_RPB = SHRINK_WAVES * SHRINK_RPW;
constexpr int EXPAND_THREADS = 256;
constexpr int LORA_MAX_R = 64;

__global__ __launch_bounds__(SHRINK_WAVES * WAVE) void lora_shrink_kernel(
    float* __restrict__ v, const short* __restrict__ x,
    const short* __restrict__ A, const int* __restrict__ ids, long x_stride,
    int K, int R, int S) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int r0 = blockIdx.y * SHRINK_RPB + wave * SHRINK_RPW;  // < R: R % 8 == 0
  float* vout = v + (long)t * R + r0;
  const int id = ids[t];
  if (id < 0 || id >= S) {
    if (lane < SHRINK_RPW) vout[lane] = 0.f;
    return;
  }
  const short* xr = x + (long)t * x_stride;
  const short* a0 = A + ((long)id * R + r0) * K;
  const short* a1 = a0 + K;
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 2
  for (int i = lane * 8; i < K; i += WAVE * 8) {
    const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xr + i);
    const bf16x8 av0 = *reinterpret_cast<const bf16x8*>(a0 + i);
    const bf16x8 av1 = *reinterpret_cast<const bf16x8*>(a1 + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xf = bits2f(xv[j]);
      acc0 = fmaf(bits2f(av0[j]), xf, acc0);
      acc1 = fmaf(bits2f(av1[j]), xf, acc1);
    }
  }
  acc0 = wave_sum(acc0);
  acc1 = wave_sum(acc1);
  if (lane == 0) {
    vout[0] = acc0;
    vout[1] = acc1;
  }
}

// RC > 0: compile-time R/8, v register-resident; RC == 0: runtime R, v
// read from LDS (broadcast) inside the loop.
template <int RC>
__global__ __launch_bounds__(EXPAND_THREADS) void lora_expand_add_kernel(
    short* __restrict__ y, const float* __restrict__ v,
    const short* __restrict__ B, const int* __restrict__ ids, long y_stride,
    int N, int R, int S) {
  __shared__ float sv[LORA_MAX_R];
  const int t = blockIdx.x;
  const int id = ids[t];
  if (id < 0 || id >= S) return;  // block-uniform: before the barrier
  const int tid = threadIdx.x;
  if (tid < R) sv[tid] = v[(long)t * R + tid];
  __syncthreads();
  const int n0 = (blockIdx.y * EXPAND_THREADS + tid) * 8;
  if (n0 >= N) return;  // N % 8 == 0: a thread's 8 columns are all in or out
  const int rc = RC > 0 ? RC : R / 8;
  float vr[RC > 0 ? RC * 8 : 1];
  if constexpr (RC > 0) {
#pragma unroll
    for (int k = 0; k < RC * 8; ++k) vr[k] = sv[k];
  }
  short* yp = y + (long)t * y_stride + n0;
  const short* bp = B + ((long)id * N + n0) * R;
  const bf16x8 yv = *reinterpret_cast<const bf16x8*>(yp);
  bf16x8 ov;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float acc = 0.f;
    if constexpr (RC > 0) {
#pragma unroll
      for (int c = 0; c < RC; ++c) {
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bp + j * R + c * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          acc = fmaf(bits2f(bv[k]), vr[c * 8 + k], acc);
      }
    } else {
      for (int c = 0; c < rc; ++c) {
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bp + j * R + c * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          acc = fmaf(bits2f(bv[k]), sv[c * 8 + k], acc);
      }
    }
    ov[j] = f2bits(bits2f(yv[j]) + acc);
  }
  *reinterpret_cast<bf16x8*>(yp) = ov;
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

void check_ids(const torch::Tensor& ids, const torch::Tensor& like, long T,
               const char* op) {
  TORCH_CHECK(ids.scalar_type() == at::kInt && ids.dim() == 1 &&
                  ids.size(0) == T && ids.is_contiguous(),
              op, ": ids must be contiguous int32 [T]");
  TORCH_CHECK(ids.device() == like.device(), op, ": ids on another device");
}

}  // namespace

void lora_shrink(torch::Tensor v, torch::Tensor x, torch::Tensor A,
                 torch::Tensor ids) {
  TORCH_CHECK(x.is_cuda() && A.is_cuda() && v.is_cuda() && ids.is_cuda(),
              "lora_shrink: GPU tensors only");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                  A.scalar_type() == at::kBFloat16,
              "lora_shrink: x and A are bf16");
  TORCH_CHECK(v.scalar_type() == at::kFloat, "lora_shrink: v is f32");
  TORCH_CHECK(x.dim() == 2 && A.dim() == 3 && v.dim() == 2,
              "lora_shrink: x [T,K], A [S,R,K], v [T,R]");
  const long T = x.size(0), K = x.size(1);
  const long S = A.size(0), R = A.size(1);
  TORCH_CHECK(A.size(2) == K, "lora_shrink: A's K differs from x's");
  TORCH_CHECK(v.size(0) == T && v.size(1) == R, "lora_shrink: v must be [T,R]");
  TORCH_CHECK(K % 256 == 0, "lora_shrink: K must be a multiple of 256");
  TORCH_CHECK(R % 8 == 0 && R >= 8 && R <= LORA_MAX_R,
              "lora_shrink: R must be a multiple of 8, at most 64");
  TORCH_CHECK(A.is_contiguous() && v.is_contiguous(),
              "lora_shrink: A and v must be contiguous");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) >= K && x.stride(0) % 8 == 0 &&
                  aligned16(x) && aligned16(A),
              "lora_shrink: x rows must be dense and 16-byte aligned");
  check_ids(ids, x, T, "lora_shrink");
  if (T == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(lora_shrink_kernel, dim3((unsigned)T, (unsigned)(R / SHRINK_RPB)),
                     dim3(SHRINK_WAVES * WAVE), 0, stream, v.data_ptr<float>(),
                     (const short*)x.data_ptr(), (const short*)A.data_ptr(),
                     ids.data_ptr<int>(), (long)x.stride(0), (int)K, (int)R,
                     (int)S);
}

void lora_expand_add(torch::Tensor y, torch::Tensor v, torch::Tensor B,
                     torch::Tensor ids) {
  TORCH_CHECK(y.is_cuda() && B.is_cuda() && v.is_cuda() && ids.is_cuda(),
              "lora_expand_add: GPU tensors only");
  TORCH_CHECK(y.scalar_type() == at::kBFloat16 &&
                  B.scalar_type() == at::kBFloat16,
              "lora_expand_add: y and B are bf16");
  TORCH_CHECK(v.scalar_type() == at::kFloat, "lora_expand_add: v is f32");
  TORCH_CHECK(y.dim() == 2 && B.dim() == 3 && v.dim() == 2,
              "lora_expand_add: y [T,N], B [S,N,R], v [T,R]");
  const long T = y.size(0), N = y.size(1);
  const long S = B.size(0), R = B.size(2);
  TORCH_CHECK(B.size(1) == N, "lora_expand_add: B's N differs from y's");
  TORCH_CHECK(v.size(0) == T && v.size(1) == R,
              "lora_expand_add: v must be [T,R]");
  TORCH_CHECK(N % 8 == 0, "lora_expand_add: N must be a multiple of 8");
  TORCH_CHECK(R % 8 == 0 && R >= 8 && R <= LORA_MAX_R,
              "lora_expand_add: R must be a multiple of 8, at most 64");
  TORCH_CHECK(B.is_contiguous() && v.is_contiguous(),
              "lora_expand_add: B and v must be contiguous");
  TORCH_CHECK(y.stride(1) == 1 && y.stride(0) >= N && y.stride(0) % 8 == 0 &&
                  aligned16(y) && aligned16(B),
              "lora_expand_add: y rows must be dense and 16-byte aligned");
  check_ids(ids, y, T, "lora_expand_add");
  if (T == 0) return;
  const long groups = N / 8;
  const dim3 grid((unsigned)T,
                  (unsigned)((groups + EXPAND_THREADS - 1) / EXPAND_THREADS));
  TORCH_CHECK(grid.y <= 65535, "lora_expand_add: N too large");
  auto stream = at::hip::getCurrentHIPStream();
#define LEA_LAUNCH(RC)                                                         \
  hipLaunchKernelGGL((lora_expand_add_kernel<RC>), grid, dim3(EXPAND_THREADS), \
                     0, stream, (short*)y.data_ptr(), v.data_ptr<float>(),     \
                     (const short*)B.data_ptr(), ids.data_ptr<int>(),          \
                     (long)y.stride(0), (int)N, (int)R, (int)S)
  switch (R) {
    case 8: LEA_LAUNCH(1); break;
    case 16: LEA_LAUNCH(2); break;
    case 32: LEA_LAUNCH(4); break;
    case 48: LEA_LAUNCH(6); break;
    default: LEA_LAUNCH(0); break;
  }
#undef LEA_LAUNCH
}
