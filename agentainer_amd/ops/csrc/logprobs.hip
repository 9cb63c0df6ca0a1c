// Per-token logprobs (gfx950): log-softmax of the model's own distribution
// plus an exact top-K (K <= 20) of each requested row, straight from the
// bf16 logits. The semantics are ops/reference.py::token_logprobs.
//
// One 1024-thread block per requested row r, b = rows[r]. The row is read
// in place (no gathered copy, no f32 workspace) three times; after the
// first read its 256 KB sit in L2:
//   1. max, and a 256-bin histogram of the high byte of the 16-bit order
//      key of each logit
//   2. sum of exp(l - max), and the histogram of the low byte among the
//      logits whose high byte is the bin that holds the K-th largest
//   3. harvest: every logit above the K-th key, and the threshold ties in
//      id order, by wave ballots over contiguous id ranges
// and one wave orders the <= 20 candidates on (value desc, id asc).
// With K = 0 only the max and the exp-sum are computed (two reads).
//
// The high byte of a bf16 is sign + 7 exponent bits, so real logits fall
// into a handful of bins and a plain LDS histogram would serialise on
// them. Each bin therefore has 32 copies, one per LDS bank: a thread adds
// to copy tid % 32, so the 32 lanes that one ds_add services together hit
// 32 different banks whatever the data is.
//
// Determinism: the histograms are integer counts, the max is exact, the
// exp-sum is accumulated per thread in id order and combined by a fixed
// shuffle tree and a fixed order over the waves, candidate slots come
// from ballots, and the final order is total. The output is a function of
// the inputs alone.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cfloat>
#include <climits>
#include "common.h"

namespace {

constexpr int NT = 1024;      // threads per block
constexpr int NW = NT / 64;   // waves per block
constexpr int KMAX = 20;      // largest top_logprobs
constexpr int BINS = 256;     // radix bins per pass (8 bits)
constexpr int COPIES = 32;    // copies of each bin, one per LDS bank

// 16-bit key of a bf16 that orders like the float does: larger value,
// larger key. -0 is folded onto +0 first, so the two tie. Any bit pattern
// (NaN included) maps into [0, 0xFFFF].
__device__ __forceinline__ unsigned key16(short s) {
  unsigned u = (unsigned short)s;
  if (u == 0x8000u) u = 0u;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}

// Visit every element of one bf16 row with 16-byte loads: `head` scalars
// up to the first 16-byte boundary, the vector body with four loads in
// flight per thread, then a scalar tail.
template <typename F>
__device__ __forceinline__ void for_row(const short* __restrict__ lp, int V,
                                        int head, F f) {
  const int tid = threadIdx.x;
  if (tid < head) f(lp[tid], tid);
  const int nvec = (V - head) / 8;
  const bf16x8* src = reinterpret_cast<const bf16x8*>(lp + head);
  auto visit = [&](const bf16x8 v, int g) {
    const int i = head + g * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) f(v[j], i + j);
  };
  int g = tid;
  for (; g + 3 * NT < nvec; g += 4 * NT) {
    const bf16x8 v0 = src[g], v1 = src[g + NT], v2 = src[g + 2 * NT],
                 v3 = src[g + 3 * NT];
    visit(v0, g); visit(v1, g + NT); visit(v2, g + 2 * NT); visit(v3, g + 3 * NT);
  }
  for (; g < nvec; g += NT) visit(src[g], g);
  for (int i = head + nvec * 8 + tid; i < V; i += NT) f(lp[i], i);
}

struct Shared {
  unsigned hist[BINS * COPIES];  // 32 KB
  unsigned bins[BINS];
  float red[NW];
  unsigned sel_bin, sel_need;
  // harvest: per wave, [0] tokens above the threshold key, [1] ties
  int w_id[NW][2][KMAX];
  int w_bits[NW][2][KMAX];
  int w_cnt[NW][2];
  int cand_id[KMAX];
  int cand_bits[KMAX];
};

// Among the tokens counted in s.hist, find the bin that holds the
// `need`-th largest; returns it and how many of that bin's tokens are
// still needed. All threads call it; s.hist may be rewritten afterwards.
__device__ __forceinline__ void select_bin(Shared& s, unsigned need,
                                           unsigned& bin, unsigned& left) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  __syncthreads();
  if (tid < BINS) {
    unsigned c = 0;
    // rotate the copy index so that 32 neighbouring bins read 32 banks
#pragma unroll
    for (int j = 0; j < COPIES; ++j)
      c += s.hist[tid * COPIES + ((j + tid) & (COPIES - 1))];
    s.bins[tid] = c;
  }
  if (tid == 0) { s.sel_bin = 0; s.sel_need = 1; }
  __syncthreads();
  if (tid < 64) {
    // lane l owns bins [4*(63-l), 4*(63-l)+3]: lanes ascend as bins
    // descend, so an inclusive lane scan counts tokens from the top
    const int b0 = (63 - lane) * 4;
    const unsigned c = s.bins[b0] + s.bins[b0 + 1] + s.bins[b0 + 2] +
                       s.bins[b0 + 3];
    unsigned incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off, WAVE);
      if (lane >= off) incl += t;
    }
    unsigned acc = incl - c;
    if (acc < need && need <= incl) {
      for (int b = b0 + 3; b >= b0; --b) {
        const unsigned h = s.bins[b];
        if (acc + h >= need) {
          s.sel_bin = (unsigned)b;
          s.sel_need = need - acc;
          break;
        }
        acc += h;
      }
    }
  }
  __syncthreads();
  bin = s.sel_bin;
  left = s.sel_need;
}

__global__ __launch_bounds__(NT) void token_logprobs_kernel(
    float* __restrict__ chosen_lp, int* __restrict__ top_id,
    float* __restrict__ top_lp, const short* __restrict__ logits,
    const int* __restrict__ rows, const long* __restrict__ chosen, int B,
    int V, int K) {
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int b = rows[r];
  if (b < 0 || b >= B) {  // not a row of logits: nothing is read
    if (tid == 0) chosen_lp[r] = __int_as_float(0x7FC00000);
    if (tid < K) { top_id[r * K + tid] = -1; top_lp[r * K + tid] = -INFINITY; }
    return;
  }
  const short* lp = logits + (long)b * V;
  // elements up to the first 16-byte boundary of the row
  int head = (int)(((16 - ((uintptr_t)lp & 15)) & 15) >> 1);
  if (head > V) head = V;
  const int Kp = K < V ? K : V;  // tokens to select

  __shared__ Shared s;

  // ---- pass 1: max, histogram of the key's high byte ---------------------
  if (Kp > 0) {
    for (int i = tid; i < BINS * COPIES; i += NT) s.hist[i] = 0;
    __syncthreads();
  }
  const int copy = tid & (COPIES - 1);
  float mx = -INFINITY;
  if (Kp > 0) {
    for_row(lp, V, head, [&](short e, int) {
      mx = fmaxf(mx, bits2f(e));
      atomicAdd(&s.hist[(key16(e) >> 8) * COPIES + copy], 1u);
    });
  } else {
    for_row(lp, V, head, [&](short e, int) { mx = fmaxf(mx, bits2f(e)); });
  }
  mx = wave_max(mx);
  if (lane == 0) s.red[wave] = mx;
  unsigned hi_bin = 0, need = (unsigned)Kp;
  if (Kp > 0) {
    select_bin(s, need, hi_bin, need);  // syncs: s.red is visible after it
    for (int i = tid; i < BINS * COPIES; i += NT) s.hist[i] = 0;
  }
  __syncthreads();
  mx = s.red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) mx = fmaxf(mx, s.red[w]);
  __syncthreads();

  // ---- pass 2: exp-sum, histogram of the low byte inside hi_bin ----------
  float sum = 0.f;
  if (Kp > 0) {
    for_row(lp, V, head, [&](short e, int) {
      sum += __expf(bits2f(e) - mx);
      const unsigned k = key16(e);
      if ((k >> 8) == hi_bin) atomicAdd(&s.hist[(k & 255u) * COPIES + copy], 1u);
    });
  } else {
    for_row(lp, V, head, [&](short e, int) { sum += __expf(bits2f(e) - mx); });
  }
  sum = wave_sum(sum);
  if (lane == 0) s.red[wave] = sum;
  unsigned lo_bin = 0;
  if (Kp > 0) select_bin(s, need, lo_bin, need);
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) total += s.red[w];
  const float lg = logf(total);  // lp[i] = (l[i] - mx) - lg

  if (tid == 0) {
    const long c = chosen[b];
    chosen_lp[r] = (c >= 0 && c < V) ? (bits2f(lp[c]) - mx) - lg
                                     : __int_as_float(0x7FC00000);
  }
  if (tid >= Kp && tid < K) {  // slots past V
    top_id[r * K + tid] = -1;
    top_lp[r * K + tid] = -INFINITY;
  }
  if (Kp == 0) return;

  // ---- pass 3: harvest ----------------------------------------------------
  // kth is the key of the Kp-th largest logit; `need` of the tokens with
  // exactly that key belong to the top Kp, the lowest ids first
  const unsigned kth = (hi_bin << 8) | lo_bin;
  const int G = Kp - (int)need;  // tokens strictly above kth
  // Each wave walks a contiguous id range in id order and keeps, in its
  // own list, what it meets above kth and its first `need` ties.
  int run_gt = 0, run_tie = 0;  // wave-uniform counts so far
  // One group: lane l holds n (<= 8) consecutive ids from id0 on; groups
  // and lanes ascend with the ids.
  auto emit = [&](const short* e, int n, int id0) {
    unsigned mg = 0, mt = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < n) {
        const unsigned k = key16(e[j]);
        mg |= (unsigned)(k > kth) << j;
        mt |= (unsigned)(k == kth) << j;
      }
    }
    if (__ballot((mg | mt) != 0) == 0ull) return;  // the common case
    const int cnt = __popc(mg) | (__popc(mt) << 16);
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, WAVE);
      if (lane >= off) incl += t;
    }
    const int excl = incl - cnt;
    const int all = __shfl(incl, 63, WAVE);
    int sg = run_gt + (excl & 0xFFFF), st = run_tie + (excl >> 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if ((mg >> j) & 1u) {
        if (sg < KMAX) { s.w_id[wave][0][sg] = id0 + j; s.w_bits[wave][0][sg] = e[j]; }
        ++sg;
      }
      if ((mt >> j) & 1u) {
        if (st < (int)need) { s.w_id[wave][1][st] = id0 + j; s.w_bits[wave][1][st] = e[j]; }
        ++st;
      }
    }
    run_gt += all & 0xFFFF;
    run_tie += all >> 16;
  };

  const int nvec = (V - head) / 8;
  if (wave == 0 && head > 0) {
    short e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int n = lane < head ? 1 : 0;
    if (n) e[0] = lp[lane];
    emit(e, n, lane);
  }
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(lp + head);
    const int Q = (nvec + NW - 1) / NW;
    const int v0 = wave * Q < nvec ? wave * Q : nvec;
    const int v1 = v0 + Q < nvec ? v0 + Q : nvec;
    for (int g0 = v0; g0 < v1; g0 += 256) {
      // four 64-vector groups per trip: the loads go out together, the
      // ballots then run group by group in id order
      bf16x8 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int g = g0 + q * 64 + lane;
        v[q] = g < v1 ? src[g] : bf16x8{};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int g = g0 + q * 64 + lane;
        short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = v[q][j];
        emit(e, g < v1 ? 8 : 0, head + g * 8);
      }
    }
  }
  if (wave == NW - 1) {
    const int t0 = head + nvec * 8;  // fewer than 8 elements remain
    if (t0 < V) {
      short e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      const int n = t0 + lane < V ? 1 : 0;
      if (n) e[0] = lp[t0 + lane];
      emit(e, n, t0 + lane);
    }
  }
  if (lane == 0) { s.w_cnt[wave][0] = run_gt; s.w_cnt[wave][1] = run_tie; }
  __syncthreads();

  // merge the wave lists in wave (= id) order: above-threshold tokens fill
  // [0, G), the ties [G, Kp)
  {
    int off_gt = 0, off_tie = G;
    for (int w = 0; w < wave; ++w) { off_gt += s.w_cnt[w][0]; off_tie += s.w_cnt[w][1]; }
    if (lane < KMAX) {
      if (lane < run_gt && off_gt + lane < G) {
        s.cand_id[off_gt + lane] = s.w_id[wave][0][lane];
        s.cand_bits[off_gt + lane] = s.w_bits[wave][0][lane];
      }
      if (lane < run_tie && lane < (int)need && off_tie + lane < Kp) {
        s.cand_id[off_tie + lane] = s.w_id[wave][1][lane];
        s.cand_bits[off_tie + lane] = s.w_bits[wave][1][lane];
      }
    }
  }
  __syncthreads();

  // ---- order the candidates: rank on (key desc, id asc) ------------------
  if (tid < Kp) {
    const int id = s.cand_id[tid];
    const short e = (short)s.cand_bits[tid];
    const unsigned k = key16(e);
    int rank = 0;
    for (int j = 0; j < Kp; ++j) {
      const unsigned kj = key16((short)s.cand_bits[j]);
      const int idj = s.cand_id[j];
      rank += (kj > k) || (kj == k && idj < id);
    }
    top_id[r * K + rank] = id;
    top_lp[r * K + rank] = (bits2f(e) - mx) - lg;
  }
}

}  // namespace

void token_logprobs(torch::Tensor chosen_lp, torch::Tensor top_id,
                    torch::Tensor top_lp, torch::Tensor logits,
                    torch::Tensor rows, torch::Tensor chosen, long K) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() &&
              logits.scalar_type() == at::kBFloat16,
              "token_logprobs: logits must be contiguous bf16 [B, V]");
  const long B = logits.size(0), V = logits.size(1);
  const long R = rows.numel();
  TORCH_CHECK(K >= 0 && K <= KMAX, "token_logprobs: K outside [0, 20]");
  TORCH_CHECK(V >= 1 && V < INT_MAX - 8 * NT && B < INT_MAX &&
              B * V < (1L << 40) && R * (K > 0 ? K : 1) < INT_MAX);
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.is_contiguous());
  TORCH_CHECK(chosen.scalar_type() == at::kLong && chosen.is_contiguous() &&
              chosen.numel() == B);
  TORCH_CHECK(chosen_lp.scalar_type() == at::kFloat &&
              chosen_lp.is_contiguous() && chosen_lp.numel() == R);
  TORCH_CHECK(top_id.scalar_type() == at::kInt && top_id.is_contiguous() &&
              top_id.numel() == R * K);
  TORCH_CHECK(top_lp.scalar_type() == at::kFloat && top_lp.is_contiguous() &&
              top_lp.numel() == R * K);
  for (const auto& t : {chosen_lp, top_id, top_lp, rows, chosen})
    TORCH_CHECK(t.device() == logits.device(),
                "token_logprobs: device mismatch");
  if (R == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      token_logprobs_kernel, dim3(R), dim3(NT), 0, stream,
      chosen_lp.data_ptr<float>(), top_id.data_ptr<int>(),
      top_lp.data_ptr<float>(), (const short*)logits.data_ptr(),
      rows.data_ptr<int>(), (const long*)chosen.data_ptr(), (int)B, (int)V,
      (int)K);
}
