// Extended sampler (gfx950): penalties + logit_bias + top-k / min-p / top-p.
//
// One 256-thread block per row, as greedy_kernel / topp_kernel. The
// semantics are defined by ops/reference.py::sample_ex; in short, per row:
//   1. the bf16 logits are widened to f32 into the workspace row ws[row]
//   2. the row's sparse edits (CSR: unique token, 2*count+in_prompt, bias)
//      and the still-in-flight pending token are applied to ws
//   3. temperature <= 0: argmax of ws, lowest id on ties
//   4. else p = exp(l/T - max), total = sum p over the whole row, and an
//      EXACT top-n0 selection (n0 = min(top_k or 1024, 1024, V)) by a
//      3 x 10-bit radix select on the bit pattern of p (the first
//      histogram is built in the exp-sum pass), ties at the threshold
//      taken in id order
//   5. the <= 1024 candidates are bitonic-sorted in LDS on (p desc, id asc),
//      cut by top-k / min-p / top-p and drawn by inverse CDF
//
// Determinism: the only atomics are integer LDS histogram counts and
// atomicMin, both order-independent; candidate slots come from wave
// ballots over fixed id ranges and the sort key is a total order, so the
// output is a function of the inputs alone. There is no fallback that
// drops a filter: a nucleus wider than 1024 tokens is truncated to the
// top 1024 (topp_kernel truncates at 512).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cfloat>
#include <climits>
#include "common.h"

namespace {

constexpr int CAP = 1024;     // candidate capacity (LDS sort width)
constexpr int NT = 256;       // threads per block
constexpr int RBINS = 1024;   // radix-select bins per pass (10 bits)
constexpr unsigned KEY_ONE = 0x3F800000u;  // bits of 1.0f: p <= 1 < 2^30

// Visit every element of one f32 row with 16-byte loads. `head` scalars
// come first so that w + head is 16-byte aligned (the row starts at an
// arbitrary element offset when V is not a multiple of 4); a scalar tail
// covers the rest.
template <typename F>
__device__ __forceinline__ void for_row(const float* __restrict__ w, int V,
                                        int head, F f) {
  const int tid = threadIdx.x;
  if (tid < head) f(w[tid], tid);
  const int nvec = (V - head) / 4;
  const f32x4* wv = reinterpret_cast<const f32x4*>(w + head);
  auto visit = [&](const f32x4 v, int g) {
    const int i = head + g * 4;
    f(v[0], i); f(v[1], i + 1); f(v[2], i + 2); f(v[3], i + 3);
  };
  // one block per row leaves 4 waves on a CU: keep 4 loads in flight per
  // thread, or every pass is bound by load latency
  int g = tid;
  for (; g + 3 * NT < nvec; g += 4 * NT) {
    const f32x4 v0 = wv[g], v1 = wv[g + NT], v2 = wv[g + 2 * NT],
                v3 = wv[g + 3 * NT];
    visit(v0, g); visit(v1, g + NT); visit(v2, g + 2 * NT); visit(v3, g + 3 * NT);
  }
  for (; g < nvec; g += NT) visit(wv[g], g);
  for (int i = head + nvec * 4 + tid; i < V; i += NT) f(w[i], i);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Radix key of a token: the bit pattern of p = exp(l/T - max), which is
// monotone in p for p >= 0. Clamped to bits(1.0f) so that a NaN logit can
// never index past the histogram.
__device__ __forceinline__ unsigned pkey(float l, float invT, float mx) {
  const unsigned k = __float_as_uint(__expf(l * invT - mx));
  return k < KEY_ONE ? k : KEY_ONE;
}

// (p descending, id ascending): true when a sorts strictly before b
__device__ __forceinline__ bool before(float pa, int ia, float pb, int ib) {
  return pa > pb || (pa == pb && ia < ib);
}

__global__ __launch_bounds__(NT) void sample_ex_kernel(
    long* __restrict__ out, const short* __restrict__ logits,
    float* __restrict__ ws, const float* __restrict__ temps,
    const float* __restrict__ top_ps, const float* __restrict__ min_ps,
    const float* __restrict__ reps, const float* __restrict__ press,
    const float* __restrict__ freqs, const int* __restrict__ top_ks,
    const unsigned long long* __restrict__ seeds,
    const int* __restrict__ edit_ptr, const int* __restrict__ edit_tok,
    const int* __restrict__ edit_cnt, const float* __restrict__ edit_bias,
    const long* __restrict__ pending_tok, int V, int nnz) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long base = (long)row * V;
  const short* lp = logits + base;
  float* w = ws + base;
  // elements up to the first multiple of 8 of the flat index: past them
  // both the bf16 row (16 B) and the f32 row (32 B) are vector-aligned
  int head = (int)((8 - (base & 7)) & 7);
  if (head > V) head = V;

  __shared__ float red[4];
  __shared__ float cand_p[CAP];
  __shared__ int cand_i[CAP];
  __shared__ float cum[CAP];
  __shared__ unsigned hist[RBINS];
  __shared__ unsigned sel_prefix, sel_need;
  __shared__ int wcnt_gt[4], wcnt_tie[4];
  __shared__ int pend_found;
  __shared__ int n_minp_s, n_topp_s, pick_s;
  __shared__ float wtot[4];
  __shared__ float bestv[4];
  __shared__ int besti[4];

  // ---- 1. widen the row into the workspace -----------------------------
  if (tid < head) w[tid] = bits2f(lp[tid]);
  {
    const int nvec = (V - head) / 8;
    const bf16x8* src = reinterpret_cast<const bf16x8*>(lp + head);
    auto widen = [&](const bf16x8 v, int g) {
      f32x4 a, b;
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = bits2f(v[j]); b[j] = bits2f(v[4 + j]); }
      f32x4* dst = reinterpret_cast<f32x4*>(w + head + g * 8);
      dst[0] = a;
      dst[1] = b;
    };
    int g = tid;
    for (; g + 3 * NT < nvec; g += 4 * NT) {
      const bf16x8 v0 = src[g], v1 = src[g + NT], v2 = src[g + 2 * NT],
                   v3 = src[g + 3 * NT];
      widen(v0, g); widen(v1, g + NT); widen(v2, g + 2 * NT); widen(v3, g + 3 * NT);
    }
    for (; g < nvec; g += NT) widen(src[g], g);
    for (int i = head + nvec * 8 + tid; i < V; i += NT) w[i] = bits2f(lp[i]);
  }
  if (tid == 0) { pend_found = 0; sel_prefix = 0; sel_need = 1; }
  __syncthreads();

  // ---- 2. sparse edits + the in-flight token ---------------------------
  const float rep = reps[row], pres = press[row], freq = freqs[row];
  const long pend = pending_tok[row];
  {
    int e0 = edit_ptr[row], e1 = edit_ptr[row + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;
    for (int e = e0 + tid; e < e1; e += NT) {
      const int tok = edit_tok[e];
      if (tok < 0 || tok >= V) continue;
      int cnt = edit_cnt[e];
      if ((long)tok == pend) { cnt += 2; pend_found = 1; }
      const int c = cnt >> 1;
      float l = w[tok];
      if (cnt > 0) l = l > 0.f ? __fdiv_rn(l, rep) : __fmul_rn(l, rep);
      // explicit roundings: no fma contraction, so ws matches the f32
      // reference bit for bit
      const float pen = __fadd_rn(__fmul_rn(freq, (float)c), c > 0 ? pres : 0.f);
      l = __fsub_rn(l, pen);
      l = __fadd_rn(l, edit_bias[e]);
      w[tok] = l;
    }
  }
  __syncthreads();
  if (tid == 0 && !pend_found && pend >= 0 && pend < V) {
    // not in the CSR: a fresh (seen, c = 1, bias = 0) edit
    float l = w[pend];
    l = l > 0.f ? __fdiv_rn(l, rep) : __fmul_rn(l, rep);
    l = __fsub_rn(l, __fadd_rn(freq, pres));
    w[pend] = l;
  }
  __syncthreads();

  const float T = temps[row];
  if (T <= 0.f) {
    // ---- 3. greedy: argmax of the edited row, lowest id on ties --------
    float best = -INFINITY;
    int best_i = INT_MAX;
    for_row(w, V, head, [&](float f, int i) {
      if (f > best || (f == best && i < best_i)) { best = f; best_i = i; }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, WAVE);
      const int oi = __shfl_xor(best_i, off, WAVE);
      if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    if (lane == 0) { bestv[wave] = best; besti[wave] = best_i; }
    __syncthreads();
    if (tid == 0) {
      best = bestv[0]; best_i = besti[0];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (bestv[k] > best || (bestv[k] == best && besti[k] < best_i)) {
          best = bestv[k]; best_i = besti[k];
        }
      out[row] = best_i < V ? best_i : 0;
    }
    return;
  }

  // ---- 4. softmax statistics --------------------------------------------
  const float invT = 1.0f / T;
  float mx = -FLT_MAX;
  for_row(w, V, head, [&](float f, int) { mx = fmaxf(mx, f * invT); });
  mx = block_max(mx, red);
  // exp-sum, and in the same pass the histogram of the top 10 key bits
  // (radix pass 0)
  for (int i = tid; i < RBINS; i += NT) hist[i] = 0;
  __syncthreads();
  float sum = 0.f;
  for_row(w, V, head, [&](float f, int) {
    const unsigned k = pkey(f, invT, mx);
    sum += __uint_as_float(k);
    atomicAdd(&hist[k >> 20], 1u);
  });
  const float total = block_sum(sum, red);

  int n0 = top_ks[row];
  if (n0 <= 0 || n0 > CAP) n0 = CAP;
  if (n0 > V) n0 = V;

  // ---- exact top-n0: radix select on the 30 significant key bits --------
  // after the loop `prefix` is the key of the n0-th largest p and `need`
  // is how many tokens with exactly that key belong to the top n0
  unsigned prefix = 0, need = (unsigned)n0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = 20 - 10 * pass;
    if (pass > 0) {
      for (int i = tid; i < RBINS; i += NT) hist[i] = 0;
      __syncthreads();
      for_row(w, V, head, [&](float f, int) {
        const unsigned k = pkey(f, invT, mx);
        if ((k >> (shift + 10)) == prefix)
          atomicAdd(&hist[(k >> shift) & (RBINS - 1)], 1u);
      });
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns bins [16*(63-l), 16*(63-l)+15]: lanes ascend as bins
      // descend, so an inclusive lane scan counts tokens from the top
      const int b0 = (63 - lane) * 16;
      unsigned s = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += hist[b0 + j];
      unsigned incl = s;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += t;
      }
      unsigned acc = incl - s;
      if (acc < need && need <= incl) {
        for (int b = b0 + 15; b >= b0; --b) {
          const unsigned h = hist[b];
          if (acc + h >= need) {
            sel_prefix = (prefix << 10) | (unsigned)b;
            sel_need = need - acc;
            break;
          }
          acc += h;
        }
      }
    }
    __syncthreads();
    prefix = sel_prefix;
    need = sel_need;
  }
  const unsigned kth = prefix;
  const int G = n0 - (int)need;  // tokens strictly above the threshold key

  // ---- harvest: each wave owns a contiguous id range; slots come from
  // ballots, so greater-than tokens land in [0, G) and threshold ties in
  // [G, n0) in id order, with no arrival-order dependence ----------------
  const int Q = (V + 3) / 4;
  const int lo = wave * Q;
  const int hi = (lo + Q < V) ? lo + Q : V;
  {
    int cg = 0, ct = 0;
    int i = lo + lane;
    for (; i + 192 < hi; i += 256) {
      const float f0 = w[i], f1 = w[i + 64], f2 = w[i + 128], f3 = w[i + 192];
      const unsigned k0 = pkey(f0, invT, mx), k1 = pkey(f1, invT, mx),
                     k2 = pkey(f2, invT, mx), k3 = pkey(f3, invT, mx);
      cg += (k0 > kth) + (k1 > kth) + (k2 > kth) + (k3 > kth);
      ct += (k0 == kth) + (k1 == kth) + (k2 == kth) + (k3 == kth);
    }
    for (; i < hi; i += 64) {
      const unsigned k = pkey(w[i], invT, mx);
      cg += k > kth;
      ct += k == kth;
    }
    cg = wave_sum_i(cg);
    ct = wave_sum_i(ct);
    if (lane == 0) { wcnt_gt[wave] = cg; wcnt_tie[wave] = ct; }
  }
  __syncthreads();
  {
    int run_gt = 0, run_tie = G;
    for (int k = 0; k < wave; ++k) { run_gt += wcnt_gt[k]; run_tie += wcnt_tie[k]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c0 = lo; c0 < hi; c0 += 256) {
      // four 64-id groups per trip: the loads go out together, the
      // ballots then run group by group in id order
      float f[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = c0 + q * 64 + lane;
        f[q] = i < hi ? w[i] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = c0 + q * 64 + lane;
        const bool valid = i < hi;
        const unsigned k = valid ? pkey(f[q], invT, mx) : 0u;
        const bool gt = valid && k > kth;
        const bool tie = valid && k == kth;
        const unsigned long long mg = __ballot(gt);
        const unsigned long long mt = __ballot(tie);
        if (gt) {
          const int slot = run_gt + __popcll(mg & below);
          if (slot < n0) { cand_p[slot] = __uint_as_float(k); cand_i[slot] = i; }
        }
        if (tie) {
          const int slot = run_tie + __popcll(mt & below);
          if (slot < n0) { cand_p[slot] = __uint_as_float(k); cand_i[slot] = i; }
        }
        run_gt += __popcll(mg);
        run_tie += __popcll(mt);
      }
    }
  }
  int npow = 1;
  while (npow < n0) npow <<= 1;
  for (int i = n0 + tid; i < npow; i += NT) { cand_p[i] = -1.f; cand_i[i] = INT_MAX; }
  __syncthreads();

  // ---- 5. bitonic sort on the composite key (p desc, id asc) ------------
  for (int k = 2; k <= npow; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow; i += NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const float pi = cand_p[i], pj = cand_p[ixj];
          const int ii = cand_i[i], ij = cand_i[ixj];
          const bool up = (i & k) == 0;
          if (up ? before(pj, ij, pi, ii) : before(pi, ii, pj, ij)) {
            cand_p[i] = pj; cand_p[ixj] = pi;
            cand_i[i] = ij; cand_i[ixj] = ii;
          }
        }
      }
      __syncthreads();
    }
  }

  // inclusive prefix sums of the sorted p: 4 consecutive per thread
  {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid * 4 + j;
      v[j] = i < n0 ? cand_p[i] : 0.f;
    }
    v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
    float incl = v[3];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float t = __shfl_up(incl, off, WAVE);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    if (tid == 0) { n_minp_s = n0; n_topp_s = n0; }
    __syncthreads();
    float offs = 0.f;
    for (int k = 0; k < wave; ++k) offs += wtot[k];
    const float excl = offs + (incl - v[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid * 4 + j;
      if (i < n0) cum[i] = excl + v[j];
    }
  }
  __syncthreads();

  // the three cuts: top-k is n0 itself, min-p and top-p by first failure
  const float top_p = top_ps[row];
  const float p_floor = min_ps[row] * cand_p[0];
  for (int i = tid; i < n0; i += NT) {
    if (cand_p[i] < p_floor) atomicMin(&n_minp_s, i);
    if (top_p < 1.0f && cum[i] / total >= top_p) atomicMin(&n_topp_s, i + 1);
  }
  __syncthreads();
  int keep = n_minp_s < n_topp_s ? n_minp_s : n_topp_s;
  if (keep > n0) keep = n0;
  if (keep < 1) keep = 1;
  if (tid == 0) pick_s = keep - 1;
  __syncthreads();

  // inverse-CDF draw over the kept prefix
  const float u = uniform01(seeds[row], row);
  const float target = u * cum[keep - 1];
  for (int i = tid; i < keep; i += NT)
    if (cum[i] >= target) atomicMin(&pick_s, i);
  __syncthreads();
  if (tid == 0) out[row] = cand_i[pick_s];
}

}  // namespace

void sample_ex(torch::Tensor out, torch::Tensor logits, torch::Tensor ws,
               torch::Tensor temps, torch::Tensor top_ps, torch::Tensor min_ps,
               torch::Tensor reps, torch::Tensor press, torch::Tensor freqs,
               torch::Tensor top_ks, torch::Tensor seeds,
               torch::Tensor edit_ptr, torch::Tensor edit_tok,
               torch::Tensor edit_cnt, torch::Tensor edit_bias,
               torch::Tensor pending_tok) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() &&
              logits.scalar_type() == at::kBFloat16);
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && B * V < (1L << 40));
  TORCH_CHECK(out.scalar_type() == at::kLong && out.is_contiguous() &&
              out.numel() == B);
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.is_contiguous() &&
              ws.numel() >= B * V);
  TORCH_CHECK((uintptr_t)logits.data_ptr() % 16 == 0 &&
              (uintptr_t)ws.data_ptr() % 32 == 0,
              "sample_ex: logits/ws base must be vector-aligned");
  for (const auto& t : {temps, top_ps, min_ps, reps, press, freqs})
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() &&
                t.numel() == B);
  TORCH_CHECK(top_ks.scalar_type() == at::kInt && top_ks.numel() == B);
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.numel() == B);
  TORCH_CHECK(pending_tok.scalar_type() == at::kLong &&
              pending_tok.numel() == B);
  TORCH_CHECK(edit_ptr.scalar_type() == at::kInt && edit_ptr.numel() == B + 1);
  const long nnz = edit_tok.numel();
  TORCH_CHECK(edit_tok.scalar_type() == at::kInt &&
              edit_cnt.scalar_type() == at::kInt && edit_cnt.numel() == nnz &&
              edit_bias.scalar_type() == at::kFloat &&
              edit_bias.numel() == nnz && nnz < INT_MAX);
  for (const auto& t : {out, ws, temps, top_ps, min_ps, reps, press, freqs,
                        top_ks, seeds, edit_ptr, edit_tok, edit_cnt, edit_bias,
                        pending_tok})
    TORCH_CHECK(t.device() == logits.device(), "sample_ex: device mismatch");
  if (B == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      sample_ex_kernel, dim3(B), dim3(NT), 0, stream, out.data_ptr<long>(),
      (const short*)logits.data_ptr(), ws.data_ptr<float>(),
      temps.data_ptr<float>(), top_ps.data_ptr<float>(),
      min_ps.data_ptr<float>(), reps.data_ptr<float>(),
      press.data_ptr<float>(), freqs.data_ptr<float>(),
      top_ks.data_ptr<int>(), (const unsigned long long*)seeds.data_ptr(),
      edit_ptr.data_ptr<int>(), edit_tok.data_ptr<int>(),
      edit_cnt.data_ptr<int>(), edit_bias.data_ptr<float>(),
      (const long*)pending_tok.data_ptr(), (int)V, (int)nnz);
}
