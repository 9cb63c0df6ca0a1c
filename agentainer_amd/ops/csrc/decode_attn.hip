// Paged GQA decode attention (gfx950) — split-KV, one launch.
//
// Serves the concurrent-agent decode step (SURVEY.md §2.3 "Decode attention
// kernel" row; BASELINE.json configs 2-5). HBM-bound: the whole op streams
// seq_len * 2 * D bf16 of K/V per (seq, kv-head) ONCE — the GQA group's
// `ratio` query heads share every K/V byte loaded.
//
// grid (n_seqs, n_kv), SPLITS (8) waves per block. Wave w owns the w-th
// chunk-aligned KV span of its (seq, kv head) and ALL `ratio` q heads of
// that kv head (RATIO is a template constant so the per-head accumulators
// stay in registers — runtime indexing would spill to scratch).
//     score phase: lane = token. K layout [page][h][D/8][ps][8] gives
//       16-lane-contiguous 16 B loads; each loaded k-vector feeds RATIO
//       dot products against q rows broadcast from LDS.
//     PV phase: lane = dim pair; V rows read once (4 B/lane contiguous),
//       each value feeds RATIO accumulators via p broadcast from LDS.
//   Online softmax per span; the wave's unnormalized (m, l, o) go to an LDS
//   merge area, and after one barrier wave h merges the SPLITS partials of
//   head h with the standard log-sum-exp rescale, normalizes, writes bf16.
//   (The partials used to take a round trip through an HBM workspace to a
//   second kernel; the arithmetic of both halves is unchanged, bit for bit:
//   tests/test_decode_attn_golden.py.)
//
// Parallelism: B*n_kv*SPLITS waves (e.g. 64 seqs x 8 kv x 8 = 4096 waves
// on 256 CUs) — the v1 single-wave-per-(seq, head) design peaked at 2
// workgroups/CU and 0.36 TB/s; this shape exists to keep every CU's memory
// queue full. The register allocator is left uncapped (about 180 VGPRs at
// RATIO 4, one 8-wave block per CU): every build held to 128 VGPRs, for
// two blocks per CU, spilled 300 - 400 B/lane and ran 1.7x slower.
//
// Latency: every global load is unconditional (token index clamped to the
// last valid token, the mask discards the lane). With a power-of-two page
// size >= 16 (FAST) a chunk's 64 / PS page ids are wave-uniform scalar
// loads, fetched once per chunk for both phases and one chunk ahead;
// page / slot are split by shift and mask, and a K or V address is that
// scalar page base plus a 32-bit lane offset. A chunk's 16 K loads are in
// flight together; its V rows follow the softmax, 8 u-steps in flight.
// (Issuing V ahead of the softmax was measured and not taken:
// profiles/README.md.)
//
// Barriers: every __syncthreads() is reached by all waves of the block;
// the only early exit is the block-uniform seq_lens[b] <= 0 in front of
// the first one. A wave with an empty span skips its chunk loop only.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cfloat>
#include "common.h"

namespace {

constexpr int CHUNK = 64;
constexpr int SPLITS = 8;
constexpr int PART_STRIDE = 132;  // 128 o + m + l (+2 pad: 16-B rows)

// Merge of the SPLITS partials of one head: `pp` points at split 0 of the
// head, `step` floats separate the splits, a lane owns dims 2*lane, +1.
// The expressions are those of the former combine kernel, kept as written.
template <int D>
__device__ __forceinline__ void merge_partials(short* __restrict__ op,
                                               const float* pp, int step,
                                               int lane) {
  float M = -FLT_MAX;
#pragma unroll
  for (int s = 0; s < SPLITS; ++s) M = fmaxf(M, pp[s * step + 128]);
  float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
  for (int s = 0; s < SPLITS; ++s) {
    const float ms = pp[s * step + 128];
    if (ms == -FLT_MAX) continue;
    const float w = __expf(ms - M);
    L += w * pp[s * step + 129];
    O0 = fmaf(w, pp[s * step + 2 * lane], O0);
    O1 = fmaf(w, pp[s * step + 2 * lane + 1], O1);
  }
  const float inv = (L > 0.f) ? 1.0f / L : 0.f;
  op[0] = f2bits(O0 * inv);
  op[1] = f2bits(O1 * inv);
}

// CT = short (bf16 pages) or unsigned char (fp8 e4m3 pages, scale-free):
// the fp8 path reads HALF the KV bytes and pays VALU converts instead of
// v_dot2 — a good trade everywhere the kernel is HBM- or latency-bound.
// FAST: PS is a power of two >= 16 (ps_shift = log2 PS) and RATIO <= 4
// (RATIO 8 carries 64 accumulators; its FAST form spills 230 - 270 B/lane
// at 256 VGPRs, so it keeps one page lookup in front of each load).
template <int RATIO, int D, typename CT, bool FAST>
__global__ __launch_bounds__(SPLITS * WAVE) void decode_attn_kernel(
    short* __restrict__ out,            // [B, n_q, D]
    const short* __restrict__ q,        // [B, n_q, D], token stride q_ts
    const CT* __restrict__ k_cache,     // [P, n_kv, D/8, PS, 8]
    const CT* __restrict__ v_cache,     // [P, n_kv, PS, D]
    const int* __restrict__ page_table, // [B, max_pages]
    const int* __restrict__ seq_lens,   // [B]
    float scale, int n_q, int n_kv, int PS, int ps_shift, int max_pages,
    long q_ts) {
  constexpr bool FP8 = sizeof(CT) == 1;
  constexpr int D8 = D / 8;
  constexpr int VWIN = 8;  // V u-steps in flight in the PV phase
  const int b = blockIdx.x;
  const int g = blockIdx.y;
  const int split = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x % WAVE;
  const int len = seq_lens[b];
  if (len <= 0) return;  // block-uniform, in front of every barrier

  __shared__ float part_lds[SPLITS][RATIO][PART_STRIDE];
  __shared__ float p_all[SPLITS][RATIO][CHUNK];
  float (*p_lds)[CHUNK] = p_all[split];
  const int qh0 = g * RATIO;
  // score-phase lane split: ds = lane/16 owns a 32-dim slice, t16 = lane%16
  // walks tokens. The dots run on v_dot2_f32_bf16 — the previous
  // LDS-broadcast-per-element formulation was instruction-issue-bound
  // (512 ds_read + 512 fma per token).
  const int ds = lane / 16;
  const int t16 = lane % 16;
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  // lane (ds, t16) owns dims {(4r+ds)*8 .. +8} for r in 0..3: for each r
  // the wave's 64 lanes cover 4 CONSECUTIVE d8 groups x 16 consecutive
  // tokens = one contiguous 1 KB run per page (full coalescing).
  // q parks in LDS (RATIO x 256 B, staged once per block) and is read per
  // k-slice as a broadcast b128 — holding it in VGPRs cost 64 registers
  // (an occupancy level at RATIO=4).
  __shared__ short q_lds[RATIO][D];
  for (int i = threadIdx.x; i < RATIO * D; i += SPLITS * WAVE)
    q_lds[i / D][i % D] = q[(long)b * q_ts + (long)(qh0 + i / D) * D + i % D];
  __syncthreads();

  // fp8 MFMA score phase operands: q quantized per head to e4m3 in LDS
  // (B operand, row stride padded to dodge 16-way bank conflicts) plus
  // the per-head scales. Scores come from v_mfma_f32_16x16x32_fp8_fp8 —
  // CDNA4 has no VALU fp8 dot, and the cvt+fma fallback was VALU-bound
  // (225 us vs bf16's 204 at ctx 4096 despite half the bytes).
  // Once per block: wave w quantizes rows w and w + 8 of the 16.
  constexpr int Q8S = D + 8;  // bytes per padded q8 row
  __shared__ unsigned char q8_lds[FP8 ? 16 * Q8S : 1];
  __shared__ float qsc_lds[16];
  __shared__ float cm_all[SPLITS][16], cs_all[SPLITS][16], mn_all[SPLITS][16];
  if constexpr (FP8) {
#pragma unroll
    for (int hh = 0; hh < 16 / SPLITS; ++hh) {
      const int h = split + hh * SPLITS;
      float sc = 0.f;
      if (h < RATIO) {
        float mx = fmaxf(fabsf(bits2f(q_lds[h][2 * lane])),
                         fabsf(bits2f(q_lds[h][2 * lane + 1])));
        mx = wave_max(mx);
        sc = fmaxf(mx, 1e-8f) / 448.f;
        const float inv = 1.f / sc;
        q8_lds[h * Q8S + 2 * lane] =
            f2fp8(bits2f(q_lds[h][2 * lane]) * inv);
        q8_lds[h * Q8S + 2 * lane + 1] =
            f2fp8(bits2f(q_lds[h][2 * lane + 1]) * inv);
      } else {
        q8_lds[h * Q8S + 2 * lane] = 0;
        q8_lds[h * Q8S + 2 * lane + 1] = 0;
      }
      if (lane == 0) qsc_lds[h] = sc;
    }
    __syncthreads();
  }

  // PV lane split: pv_tg = lane/16 walks tokens (4 per u-step, adjacent
  // rows => 1 KB contiguous per load instruction), pv_dg = lane%16 owns
  // 8 dims (one 16 B load per row); o[RATIO][8] are the accumulators.
  const int pv_tg = lane / 16;
  const int pv_dg = lane % 16;
  float m[RATIO], l[RATIO];
  float o[RATIO][8];
#pragma unroll
  for (int h = 0; h < RATIO; ++h) {
    m[h] = -FLT_MAX; l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[h][j] = 0.f;
  }
  const int* pt = page_table + (long)b * max_pages;
  const int psm = PS - 1;

  const int n_chunks = (len + CHUNK - 1) / CHUNK;
  const int cpw = (n_chunks + SPLITS - 1) / SPLITS;  // chunks per wave
  const int c0 = split * cpw;
  const int c1 = min(c0 + cpw, n_chunks);

  // FAST: a 16-token group lies inside one page, and clamping a token to
  // len - 1 keeps it inside the (clamped) group's page, so the page of
  // group j of chunk c is pt[min(c * 64 + j * 16, len - 1) >> ps_shift]
  // for the score phase (token j*16 + t16) and the PV phase (u / 4 == j)
  // alike. Wave-uniform: scalar loads, one chunk ahead.
  int pid_n[4] = {0, 0, 0, 0};
  if constexpr (FAST) {
    if (c0 < c1) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pid_n[j] = __builtin_amdgcn_readfirstlane(
            pt[min(c0 * CHUNK + j * 16, len - 1) >> ps_shift]);
    }
  }

  using VT = typename std::conditional<FP8, u8x8, bf16x8>::type;

  for (int c = c0; c < c1; ++c) {
    int pid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pid[j] = pid_n[j];
    if constexpr (FAST) {
      // next chunk's ids (clamped: in bounds also behind the last chunk)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pid_n[j] = __builtin_amdgcn_readfirstlane(
            pt[min((c + 1) * CHUNK + j * 16, len - 1) >> ps_shift]);
    }
    const int base_tok = c * CHUNK;
    // this lane's 16-B (8-B fp8) K slice: token tok_c of 16-token group j,
    // d8 group d8. FAST: wave-uniform page base + a 32-bit lane offset.
    auto k_ptr = [&](int j, int tok_c, int d8) -> const CT* {
      if constexpr (FAST) {
        const char* base = reinterpret_cast<const char*>(
            k_cache + ((long)pid[j] * n_kv + g) * D8 * PS * 8);
        const unsigned boff =
            (unsigned)((d8 * PS + (tok_c & psm)) * 8) * (unsigned)sizeof(CT);
        return reinterpret_cast<const CT*>(base + boff);
      } else {
        const long page = pt[tok_c / PS];
        return k_cache + ((long)page * n_kv + g) * D8 * PS * 8 +
               (tok_c % PS) * 8 + (long)d8 * PS * 8;
      }
    };
    // this lane's V row slice of u-step u (token base + u*4 + pv_tg)
    auto v_ptr = [&](int u) -> const CT* {
      const int gt_c = min(base_tok + u * 4 + pv_tg, len - 1);
      if constexpr (FAST) {
        const char* base = reinterpret_cast<const char*>(
            v_cache + ((long)pid[u / 4] * n_kv + g) * PS * D);
        const unsigned boff =
            (unsigned)((gt_c & psm) * D + pv_dg * 8) * (unsigned)sizeof(CT);
        return reinterpret_cast<const CT*>(base + boff);
      } else {
        const long page = pt[gt_c / PS];
        return v_cache + (((long)page * n_kv + g) * PS + gt_c % PS) * D +
               pv_dg * 8;
      }
    };
    VT vb[16];
    // K loads of KA 16-token groups are in flight together
    constexpr int KA = FAST ? 4 : 1;

    if constexpr (FP8) {
      // MFMA score phase: S^T[16 tok x 16 head-col] per 16-token group.
      // A = K rows (lane: tok = l%16, k-dims (l/16)*8..+8 per 32-dim
      // chunk — 16 lanes x 8 B = one contiguous page-row span), B = q8
      // from LDS. C lane l holds tokens g*16 + (l/16)*4 + r of head
      // l%16. Per-head chunk stats cross lanes through small LDS
      // broadcast arrays; the m/l/alpha bookkeeping stays statically
      // indexed (a dynamic m[myh] would spill the accumulators).
      float* cm_b = cm_all[split];
      float* cs_b = cs_all[split];
      float* mn_b = mn_all[split];
      const int myh = lane % 16;
      float sv[16];  // this lane's 16 token scores for head `myh`
#pragma unroll
      for (int g0 = 0; g0 < 4; g0 += KA) {
        long ka[KA][4];
#pragma unroll
        for (int a = 0; a < KA; ++a) {
          const int tok = c * CHUNK + (g0 + a) * 16 + (lane % 16);
          const int tok_c = min(tok, len - 1);
#pragma unroll
          for (int dc = 0; dc < 4; ++dc)
            __builtin_memcpy(&ka[a][dc],
                             k_ptr(g0 + a, tok_c, dc * 4 + lane / 16), 8);
        }
#pragma unroll
        for (int a = 0; a < KA; ++a) {
          const int gt = g0 + a;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int dc = 0; dc < 4; ++dc) {
            long bq;
            __builtin_memcpy(
                &bq, &q8_lds[myh * Q8S + dc * 32 + (lane / 16) * 8], 8);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(ka[a][dc], bq,
                                                             acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) sv[gt * 4 + r] = acc[r];
        }
      }
      // mask + scale, per-head chunk max (lanes sharing l%16: xor 16/32)
      const float qs = qsc_lds[myh] * scale;
      float cmax = -FLT_MAX;
#pragma unroll
      for (int gt = 0; gt < 4; ++gt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tok = c * CHUNK + gt * 16 + (lane / 16) * 4 + r;
          const float v = (tok < len) ? sv[gt * 4 + r] * qs : -FLT_MAX;
          sv[gt * 4 + r] = v;
          cmax = fmaxf(cmax, v);
        }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 16, WAVE));
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32, WAVE));
      if (lane < 16) cm_b[myh] = cmax;
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      // statically-indexed running-max update; new maxima broadcast back
      float alpha_s[RATIO];
#pragma unroll
      for (int h = 0; h < RATIO; ++h) {
        const float mn = fmaxf(m[h], cm_b[h]);
        alpha_s[h] = (m[h] == -FLT_MAX) ? 0.f : __expf(m[h] - mn);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[h][j] *= alpha_s[h];
        m[h] = mn;
        if (lane == 0) mn_b[h] = mn;
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);
      // p = exp(s - mn) -> p_lds; per-head chunk sum via the same xor net
      const float mn_my = mn_b[myh];
      float csum = 0.f;
#pragma unroll
      for (int gt = 0; gt < 4; ++gt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = gt * 16 + (lane / 16) * 4 + r;
          const float pv = (sv[gt * 4 + r] == -FLT_MAX)
                               ? 0.f
                               : __expf(sv[gt * 4 + r] - mn_my);
          if (myh < RATIO) p_lds[myh][t] = pv;
          csum += pv;
        }
      csum += __shfl_xor(csum, 16, WAVE);
      csum += __shfl_xor(csum, 32, WAVE);
      if (lane < 16) cs_b[myh] = csum;
      __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
      for (int h = 0; h < RATIO; ++h) l[h] = l[h] * alpha_s[h] + cs_b[h];
    } else {
    float s[4][RATIO];  // [16-token sub-pass][head]
#pragma unroll
    for (int s0 = 0; s0 < 4; s0 += KA) {
      // this lane's 4 d8 groups per token: d8 = r*4 + ds (coalesced per r).
      // Unconditional: a token past the end is clamped, masked below.
      bf16x8 kv[KA][4];
#pragma unroll
      for (int a = 0; a < KA; ++a) {
        const int tok_c = min(c * CHUNK + (s0 + a) * 16 + t16, len - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          kv[a][r] = *reinterpret_cast<const bf16x8*>(
              k_ptr(s0 + a, tok_c, r * 4 + ds));
      }
#pragma unroll
      for (int a = 0; a < KA; ++a) {
      const int sub = s0 + a;
      const int tok = c * CHUNK + sub * 16 + t16;
      // keeps the q reads of one sub-pass from being held in registers
      // for the next (64 VGPRs at RATIO 4): LDS reads are cheap, an
      // occupancy level is not
      asm volatile("" ::: "memory");
      float acc[RATIO];
#pragma unroll
      for (int h = 0; h < RATIO; ++h) acc[h] = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bf2* kp2 = reinterpret_cast<const bf2*>(&kv[a][r]);
        // this lane's dims (4r+ds)*8..+8 of each head's q: broadcast
        // LDS reads (t16 lanes share the address — conflict-free)
#pragma unroll
        for (int h = 0; h < RATIO; ++h) {
          const bf16x8 qv8 = *reinterpret_cast<const bf16x8*>(
              &q_lds[h][(r * 4 + ds) * 8]);
          const bf2* qp2 = reinterpret_cast<const bf2*>(&qv8);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[h] = __builtin_amdgcn_fdot2_f32_bf16(kp2[j], qp2[j],
                                                     acc[h], false);
        }
      }
      // reduce the 4 dim-slices (lanes differing in bits 4..5)
#pragma unroll
      for (int h = 0; h < RATIO; ++h) {
        acc[h] += __shfl_xor(acc[h], 16, WAVE);
        acc[h] += __shfl_xor(acc[h], 32, WAVE);
        s[sub][h] = (tok < len) ? acc[h] * scale : -FLT_MAX;
      }
      }
    }
    // per-head online softmax update over the whole 64-token chunk
#pragma unroll
    for (int h = 0; h < RATIO; ++h) {
      float cm = fmaxf(fmaxf(s[0][h], s[1][h]), fmaxf(s[2][h], s[3][h]));
      cm = wave_max(cm);
      const float mn = fmaxf(m[h], cm);
      float psum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        const float p = (s[sub][h] == -FLT_MAX) ? 0.f : __expf(s[sub][h] - mn);
        if (ds == 0) {
          p_lds[h][sub * 16 + t16] = p;
          psum += p;
        }
      }
      const float csum = wave_sum(psum);
      const float alpha = (m[h] == -FLT_MAX) ? 0.f : __expf(m[h] - mn);
      l[h] = l[h] * alpha + csum;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[h][j] *= alpha;
      m[h] = mn;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): p_lds is written
    }

    // PV: per u-step this lane reads V[tok = base + u*4 + pv_tg]
    // [dims pv_dg*8 .. +8) — the wave covers 4 adjacent token rows x
    // full 256-B width = 1 KB contiguous; p broadcasts from LDS.
    auto pv_step = [&](int u, const VT vv) {
      const int t = u * 4 + pv_tg;
      float vf[8];
      if constexpr (FP8) {
        fp8x8_to_f32(vv, vf);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = bits2f(vv[j]);
      }
#pragma unroll
      for (int h = 0; h < RATIO; ++h) {
        const float pw = p_lds[h][t];  // 0 beyond len
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[h][j] = fmaf(pw, vf[j], o[h][j]);
      }
    };
    if constexpr (FAST) {
      // VWIN u-steps of V rows in flight: the first VWIN are issued here,
      // and each group of 4 FMA steps is preceded by the loads of the
      // group VWIN / 4 ahead. The fences pin that order, and keep the p
      // reads of later groups from being hoisted into registers.
#pragma unroll
      for (int u = 0; u < VWIN; ++u)
        vb[u] = *reinterpret_cast<const VT*>(v_ptr(u));
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = grp * 4 + VWIN; u < grp * 4 + VWIN + 4; ++u)
          if (u < 16)
            vb[u] = *reinterpret_cast<const VT*>(v_ptr(u));
#pragma unroll
        for (int u = grp * 4; u < grp * 4 + 4; ++u) pv_step(u, vb[u]);
      }
    } else {
#pragma unroll 4
      for (int u = 0; u < 16; ++u)
        pv_step(u, *reinterpret_cast<const VT*>(v_ptr(u)));
    }
  }

  // publish partials (unnormalized): reduce o across the 4 token groups
  // (lane bits 4..5), then pv_tg==0 lanes own dims [pv_dg*8, pv_dg*8+8).
  // An empty span publishes the neutral m = -FLT_MAX, l = 0 (its o is
  // never read).
#pragma unroll
  for (int h = 0; h < RATIO; ++h) {
    float* pp = part_lds[split][h];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = o[h][j];
      v += __shfl_xor(v, 16, WAVE);
      v += __shfl_xor(v, 32, WAVE);
      if (pv_tg == 0) pp[pv_dg * 8 + j] = v;
    }
    if (lane == 0) { pp[128] = m[h]; pp[129] = l[h]; }
  }
  __syncthreads();

  for (int h = split; h < RATIO; h += SPLITS)
    merge_partials<D>(out + ((long)b * n_q + qh0 + h) * D + 2 * lane,
                      part_lds[0][h], RATIO * PART_STRIDE, lane);
}

}  // namespace

void paged_decode_attention(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor page_table, torch::Tensor seq_lens,
                            double scale) {
  TORCH_CHECK(out.is_contiguous());
  TORCH_CHECK(q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(page_table.scalar_type() == at::kInt &&
              seq_lens.scalar_type() == at::kInt);
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
  const int B = q.size(0), n_q = q.size(1), D = q.size(2);
  const int n_kv = k_cache.size(1), PS = k_cache.size(3);
  const int max_pages = page_table.size(1);
  const int ratio = n_q / n_kv;
  TORCH_CHECK(D == 128, "decode attention: head_dim 128 only");
  TORCH_CHECK(n_q % n_kv == 0);
  if (B == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid(B, n_kv);
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  // page / slot by shift and mask for a power-of-two page size >= 16
  const bool fast = PS >= 16 && (PS & (PS - 1)) == 0;
  int ps_shift = 0;
  while ((1 << ps_shift) < PS) ++ps_shift;
#define LAUNCH_RATIO_CT(R, CT, F)                                              \
  hipLaunchKernelGGL((decode_attn_kernel<R, 128, CT, F>), grid,                \
                     dim3(SPLITS * WAVE), 0, stream, (short*)out.data_ptr(),   \
                     (const short*)q.data_ptr(),                               \
                     (const CT*)k_cache.data_ptr(),                            \
                     (const CT*)v_cache.data_ptr(),                            \
                     page_table.data_ptr<int>(), seq_lens.data_ptr<int>(),     \
                     (float)scale, n_q, n_kv, PS, ps_shift, max_pages,         \
                     (long)q.stride(0))
#define LAUNCH_RATIO(R, FAST_OK)                                               \
  do {                                                                         \
    if (fp8) {                                                                 \
      if (FAST_OK && fast) LAUNCH_RATIO_CT(R, unsigned char, FAST_OK);         \
      else LAUNCH_RATIO_CT(R, unsigned char, false);                           \
    } else {                                                                   \
      if (FAST_OK && fast) LAUNCH_RATIO_CT(R, short, FAST_OK);                 \
      else LAUNCH_RATIO_CT(R, short, false);                                   \
    }                                                                          \
  } while (0)
  switch (ratio) {
    case 1: LAUNCH_RATIO(1, true); break;
    case 2: LAUNCH_RATIO(2, true); break;
    case 4: LAUNCH_RATIO(4, true); break;
    case 8: LAUNCH_RATIO(8, false); break;
    default:
      TORCH_CHECK(false, "decode attention: GQA ratio must be 1/2/4/8, got ",
                  ratio);
  }
#undef LAUNCH_RATIO
#undef LAUNCH_RATIO_CT
}
