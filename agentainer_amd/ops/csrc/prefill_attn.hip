// Paged varlen causal prefill attention (gfx950, MFMA bf16).
//
// Flash-style online-softmax attention for the batched prefill phase of
// the continuous-batching scheduler (SURVEY.md §2.3 "Prefill attention
// kernel" row). Q rows are the batch's NEW tokens (varlen-packed); K/V are
// read from the paged pools, so a conversation's cached prefix is attended
// without re-prefilling it (the agent-KV-persistence contract).
//
// Geometry (one workgroup = 4 waves = one 32-row Q tile of 4 GQA heads):
//   grid: (n_q/4, n_seqs, ceil(max_qlen/32)); wave w -> head x*4+w; the q
//   tile is gridDim.z-1-z, so the tiles with the longest causal range are
//   dispatched first and the short ones fill the tail of the grid.
//   All 4 heads share one kv head (requires ratio % 4 == 0 — true for
//   Llama-3 8B/70B and Mixtral), so the K/V tiles staged in LDS are shared.
//   230 VGPRs, no AGPRs, no scratch, 42 KB LDS: 2 waves/SIMD, i.e. two
//   workgroups per CU, so one block's barrier and LDS round trips hide
//   under the other's MFMAs (3 waves/SIMD spills: Q, O, one K tile's
//   fragments and the staged chunks alone are 144 registers).
//   KV tile = 32 tokens. Per tile, per wave, per 16-row q sub-tile:
//     S^T tiles  = mfma_f32_16x16x32_bf16(A=Q, B=K)   [16 q x 16 kv] x 2
//     P -> LDS (bf16), online m/l update per q row
//     O tiles   += mfma(A=P, B=V^T)                    [16 q x 16 d] x 8
//   Both sub-tiles run S / softmax first, then one PV pass streams the V
//   fragments, so K and V fragments are never live together.
//   A (sub-tile, KV tile) pair wholly above the diagonal skips QK^T and the
//   softmax (they would give alpha = 1, P = 0) and enters PV with P = 0; a
//   pair wholly below it skips the mask compares. The arithmetic of every
//   output element is the one tests/golden/prefill_attn/ records, bit for
//   bit.
//   MFMA fragment maps (gfx950): A lane l holds A[l%16][(l/16)*8+j];
//   B lane l holds B[(l/16)*8+j][l%16]; C/D lane l holds rows (l/16)*4+r,
//   col l%16 (cdna_hip_programming.md §3).
//
// Data movement:
//   * Every global load is unconditional: a token index past the block's
//     causal end is clamped to the last valid token (its K column is
//     overwritten by the mask, its V row meets p == 0 exactly). The three
//     page ids a thread needs per tile are fetched two tiles ahead, the
//     K/V chunks one tile ahead (T14: issue early, write to LDS after the
//     MFMAs), so nothing in the tile loop waits on a dependent round trip.
//   * LDS: K tile [32][128] XOR-swizzled for the ds_read_b128 row reads
//     (G4/T2). V tile row-major [32][128] in the T10 image (b), written
//     with 16-B stores and read as the MFMA B operand with
//     ds_read_b64_tr_b16 (conflict-free both ways). Both double-buffered,
//     ONE barrier per tile. Per-wave P buffers; the P round trip waits on
//     lgkmcnt only, so the prefetch stays in flight.
//   * Row max / row sum butterflies run on DPP instead of ds_bpermute; the
//     mirror steps read a lane of the partner quad / half, which holds the
//     same bits as the xor partner.
//   * O leaves through LDS so the global stores are 16 B per lane.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cfloat>
#include "common.h"

namespace {

typedef __bf16 bf16v8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int QBLK = 32;
constexpr int KVBLK = 32;
constexpr int D = 128;
constexpr int P_STRIDE = KVBLK + 8;            // shorts; keeps 16-B alignment
constexpr int TILE_BYTES = KVBLK * D * 2;      // one K or V tile image
constexpr int K_OFF = 0;                       // 2 K buffers
constexpr int V_OFF = 2 * TILE_BYTES;          // 2 V buffers
constexpr int P_OFF = 4 * TILE_BYTES;          // per wave: 2 P buffers
constexpr int P_BYTES = 16 * P_STRIDE * 2;     // one [16 q][32+8 kv] bf16
constexpr int O_ROW = D * 2 + 16;              // epilogue row stride (bytes)
constexpr int LDS_BYTES = P_OFF + 4 * 2 * P_BYTES;
static_assert(4 * QBLK * O_ROW <= LDS_BYTES, "O staging reuses the tile LDS");

__device__ __forceinline__ int kswz(int tok, int byte_off) {
  // XOR swizzle within a K row: spread the 16-B slot by token (G4/T2)
  return byte_off ^ ((tok & 7) << 4);
}

// T10 image (b): byte offset of 16-B chunk ch (0..15) of V row `row`.
__device__ __forceinline__ int vswz(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// One DPP lane exchange inside a 16-lane row (full EXEC required).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                         0xF, 0xF, false));
}
constexpr int DPP_XOR1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141;  // lane i <- 7-i: the other quad
constexpr int DPP_MIRROR = 0x140;       // lane i <- 15-i: the other half

// Wait for this wave's outstanding LDS operations only (vmcnt 63, expcnt 7,
// lgkmcnt 0) and keep the compiler from moving LDS accesses across it.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
}

// PV for one KV tile: O[qs][dt] += P[qs] V^T[dt] for both q sub-tiles.
// The B operand of dim tile dt is two transposed reads (k-slots lg*8+0..3
// and +4..7) of the V image; voff is the lane's byte offset in smem for
// dt = 0 / first half. In image (b) the chunk XOR makes the other offsets
// voff ^ (dt << 5) and, four rows down, ^ 0x410. Fragments are streamed so
// only one is live at a time.
__device__ __forceinline__ void pv_tile(f32x4 (&o)[2][8],
                                        const bf16v8 (&pf)[2],
                                        const char* smem, int voff) {
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) {
    const int a = voff ^ (dt << 5);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(smem + a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(smem + (a ^ 0x410)));
    const bf16v8 vf = __builtin_bit_cast(
        bf16v8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[0], vf, o[0][dt],
                                                       0, 0, 0);
    o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[1], vf, o[1][dt],
                                                       0, 0, 0);
  }
}

// CT = short (bf16 pages) or unsigned char (fp8 e4m3 pages): the fp8
// path dequantizes to bf16 during LDS staging, so the MFMA pipeline and
// both LDS images are byte-identical to the bf16 build.
template <typename CT>
__device__ __forceinline__ bf16x8 load8_cache(const CT* p) {
  if constexpr (sizeof(CT) == 1) {
    const u8x8 b = *reinterpret_cast<const u8x8*>(p);
    float f[8];
    fp8x8_to_f32(b, f);
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = f2bits(f[j]);
    return r;
  } else {
    return *reinterpret_cast<const bf16x8*>(p);
  }
}

// POW2: page size is 1 << ps_shift (every shipped config); otherwise the
// page / slot split falls back to the integer divide, whose temporaries
// do not fit 2 waves/SIMD without scratch.
template <typename CT, bool POW2>
__global__ __launch_bounds__(256, POW2 ? 2 : 1) void prefill_attn_kernel(
    short* __restrict__ out,            // [Tq, n_q, D]
    const short* __restrict__ q,        // [Tq, n_q, D]
    const CT* __restrict__ k_cache,     // [P, n_kv, D/8, PS, 8]
    const CT* __restrict__ v_cache,     // [P, n_kv, PS, D]
    const int* __restrict__ page_table, // [B, max_pages]
    const int* __restrict__ seq_lens,   // [B] total context length
    const int* __restrict__ q_starts,   // [B] row offset into q
    const int* __restrict__ q_lens,     // [B]
    float scale, int n_q, int n_kv, int PS, int ps_shift, int max_pages,
    long q_ts) {
  const int qtile = gridDim.z - 1 - blockIdx.z;  // heaviest tiles first
  const int b = blockIdx.y;
  const int qlen = q_lens[b];
  if (qtile * QBLK >= qlen) return;              // whole block: EXEC stays full
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int head = blockIdx.x * 4 + wid;
  const int seq_len = seq_lens[b];
  const int ctx_start = seq_len - qlen;  // new tokens sit at the end
  const int ratio = n_q / n_kv;
  const int g = head / ratio;
  const int lane = threadIdx.x % WAVE;
  const int l16 = lane % 16;    // fragment col / A row
  const int lg = lane / 16;     // fragment k-group

  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  char* const p_buf = smem + P_OFF + wid * (2 * P_BYTES);  // one per q sub-tile

  const int* pt = page_table + (long)b * max_pages;
  const long q_row0 = q_starts[b];

  // ---- load Q fragments: [2 qsub][4 dchunk], lane l -> Q[qsub*16+l16][dc*32+lg*8 ..+8]
  // Rows past qlen read the last valid row: rows are independent and those
  // rows are never stored.
  bf16v8 qf[2][4];
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    const int qr = min(qtile * QBLK + qs * 16 + l16, qlen - 1);
    const short* p = q + (q_row0 + qr) * q_ts + (long)head * D + lg * 8;
#pragma unroll
    for (int dc = 0; dc < 4; ++dc)
      qf[qs][dc] = *reinterpret_cast<const bf16v8*>(p + dc * 32);
  }

  // ---- accumulators
  f32x4 o[2][8];  // [qsub][dim tile]
#pragma unroll
  for (int qs = 0; qs < 2; ++qs)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[qs][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2][4], l_run[2][4];
#pragma unroll
  for (int qs = 0; qs < 2; ++qs)
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[qs][r] = -FLT_MAX; l_run[qs][r] = 0.f; }

  const int max_qpos = ctx_start + min(qtile * QBLK + QBLK - 1, qlen - 1);
  const int kv_end = max_qpos + 1;
  const int n_tiles = (kv_end + KVBLK - 1) / KVBLK;

  // T14 split staging: each thread owns 2 K chunks + 2 V chunks of a tile
  // (K: token tid%32, 16-B slots tid/32 and tid/32+8; V: tokens tid/16 and
  // tid/16+16, slot tid%16). Tile t+1's GLOBAL loads issue before tile t's
  // MFMAs, the LDS writes land after them, ONE barrier per tile.
  const int tok_k = threadIdx.x % KVBLK, d8_k = threadIdx.x / KVBLK;
  const int tok_v = threadIdx.x / 16, ch_v = threadIdx.x % 16;
  const long kv_page = (long)D * PS;     // elements per (page, kv head)
  int pg_k, pg_v0, pg_v1;                // page ids of the next tile to load
  int in_k, in_v0, in_v1;                // slots inside those pages
  auto page_load = [&](int t) {
    const int kv0 = t * KVBLK;
    const int gk = min(kv0 + tok_k, kv_end - 1);
    const int gv0 = min(kv0 + tok_v, kv_end - 1);
    const int gv1 = min(kv0 + tok_v + 16, kv_end - 1);
    if constexpr (POW2) {
      const int msk = PS - 1;
      pg_k = pt[gk >> ps_shift];   in_k = gk & msk;
      pg_v0 = pt[gv0 >> ps_shift]; in_v0 = gv0 & msk;
      pg_v1 = pt[gv1 >> ps_shift]; in_v1 = gv1 & msk;
    } else {
      pg_k = pt[gk / PS];   in_k = gk % PS;
      pg_v0 = pt[gv0 / PS]; in_v0 = gv0 % PS;
      pg_v1 = pt[gv1 / PS]; in_v1 = gv1 % PS;
    }
  };
  bf16x8 st_k0, st_k1, st_v0, st_v1;
  auto stage_load = [&]() {
    const CT* kp = k_cache + ((long)pg_k * n_kv + g) * kv_page
                   + (d8_k * PS + in_k) * 8;
    st_k0 = load8_cache<CT>(kp);
    st_k1 = load8_cache<CT>(kp + 8 * PS * 8);
    st_v0 = load8_cache<CT>(v_cache + ((long)pg_v0 * n_kv + g) * kv_page
                            + in_v0 * D + ch_v * 8);
    st_v1 = load8_cache<CT>(v_cache + ((long)pg_v1 * n_kv + g) * kv_page
                            + in_v1 * D + ch_v * 8);
  };
  auto stage_write = [&](int buf) {
    char* kb = smem + K_OFF + buf * TILE_BYTES;
    char* vb = smem + V_OFF + buf * TILE_BYTES;
    const int kbyte = tok_k * (D * 2) + d8_k * 16;
    *reinterpret_cast<bf16x8*>(kb + kswz(tok_k, kbyte)) = st_k0;
    *reinterpret_cast<bf16x8*>(kb + kswz(tok_k, kbyte + 128)) = st_k1;
    *reinterpret_cast<bf16x8*>(vb + vswz(tok_v, ch_v)) = st_v0;
    *reinterpret_cast<bf16x8*>(vb + vswz(tok_v + 16, ch_v)) = st_v1;
  };

  // V^T fragment addresses (T10): in 16-lane group lg, lane 4q+p supplies
  // row lg*8 + h*4 + q, columns dt*16 + 4p..4p+3 and receives, in element
  // q', V[lg*8 + h*4 + q'][dt*16 + l16]: k-slot lg*8+j <-> token lg*8+j.
  // voff0 is that address for dt = 0, h = 0; pv_tile derives the rest.
  const int vq = l16 >> 2, vp = l16 & 3;
  const int voff0 = vswz(lg * 8 + vq, vp >> 1) + 8 * (vp & 1);

  page_load(0);
  stage_load();
  page_load(1);
  stage_write(0);
  __syncthreads();
  int buf = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * KVBLK;
    const bool has_next = (t + 1 < n_tiles);
    if (has_next) stage_load();  // next tile's HBM loads in flight
    page_load(t + 2);            // page ids for the tile after that

    const char* kb = smem + K_OFF + buf * TILE_BYTES;
    // ---- K fragments for this tile: [2 ksub][4 dchunk]
    bf16v8 kf[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int tok = ks * 16 + l16;
#pragma unroll
      for (int dc = 0; dc < 4; ++dc) {
        const int byte0 = tok * (D * 2) + (dc * 32 + lg * 8) * 2;
        kf[ks][dc] = *reinterpret_cast<const bf16v8*>(kb + kswz(tok, byte0));
      }
    }
    // Which 16-row q sub-tiles take part in this tile. Skipped: no valid
    // row, or every (row, token) pair above the diagonal — the update
    // would be alpha = 1, p = 0. Block-uniform, so EXEC stays full.
    bool act[2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      const int rb = qtile * QBLK + qs * 16;
      act[qs] = rb < qlen && kv0 <= ctx_start + min(rb + 15, qlen - 1);
    }

    // ---- phase 1: S = Q K^T, online softmax, P -> LDS, rescale O
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      if (!act[qs]) continue;
      const int rb = qtile * QBLK + qs * 16;  // first row of the sub-tile
      const bool need_mask = (kv0 + KVBLK - 1 > ctx_start + rb) ||
                             (rb + 15 >= qlen);
      // S^T tiles: [2 ksub][16q x 16kv]
      f32x4 s[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dc = 0; dc < 4; ++dc)
          s[ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[qs][dc], kf[ks][dc], s[ks], 0, 0, 0);
      }
      // scale + mask. lane holds rows (lg*4+r), col l16 (kv).
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) s[ks][r] = s[ks][r] * scale;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qr = rb + lg * 4 + r;
          const int qpos = ctx_start + qr;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int kpos = kv0 + ks * 16 + l16;
            if (qr >= qlen || kpos > qpos) s[ks][r] = -FLT_MAX;
          }
        }
      }
      // row max over the 16 lanes of a row
      float rmax[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = fmaxf(s[0][r], s[1][r]);
        mx = fmaxf(mx, dpp_mov<DPP_XOR1>(mx));
        mx = fmaxf(mx, dpp_mov<DPP_XOR2>(mx));
        mx = fmaxf(mx, dpp_mov<DPP_HALF_MIRROR>(mx));
        mx = fmaxf(mx, dpp_mov<DPP_MIRROR>(mx));
        rmax[r] = mx;
      }
      // online update
      float alpha[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(m_run[qs][r], rmax[r]);
        alpha[r] = (m_run[qs][r] == -FLT_MAX) ? 0.f : __expf(m_run[qs][r] - mn);
        m_run[qs][r] = mn;
        float rowsum = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          float p = (s[ks][r] == -FLT_MAX) ? 0.f : __expf(s[ks][r] - mn);
          s[ks][r] = p;
          rowsum += p;
        }
        rowsum += dpp_mov<DPP_XOR1>(rowsum);
        rowsum += dpp_mov<DPP_XOR2>(rowsum);
        rowsum += dpp_mov<DPP_HALF_MIRROR>(rowsum);
        rowsum += dpp_mov<DPP_MIRROR>(rowsum);
        l_run[qs][r] = l_run[qs][r] * alpha[r] + rowsum;
      }
      // P -> LDS (bf16) for the A-fragment of PV
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<short*>(
              p_buf + qs * P_BYTES +
              ((lg * 4 + r) * P_STRIDE + ks * 16 + l16) * 2) = f2bits(s[ks][r]);
      // rescale O
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[qs][dt][r] *= alpha[r];
    }

    // ---- phase 2: PV. A = P fragment (lane: P[l16][lg*8+j]) back from
    // this wave's LDS, B = V^T fragments streamed per 16-dim tile.
    wave_lds_fence();  // own-wave LDS ordering; global prefetch stays in flight
    // A skipped sub-tile takes part with P = 0: O += 0 * V, what the
    // masked update adds, and one straight-line PV serves every case.
    bf16v8 pf[2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      pf[qs] = *reinterpret_cast<const bf16v8*>(
          p_buf + qs * P_BYTES + (l16 * P_STRIDE + lg * 8) * 2);
      if (!act[qs]) pf[qs] = bf16v8{};
    }
    wave_lds_fence();  // the next tile's P stores stay behind these reads
    pv_tile(o, pf, smem, V_OFF + buf * TILE_BYTES + voff0);
    if (has_next) stage_write(buf ^ 1);  // writes land after the MFMAs
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: O /= l -> bf16 -> this wave's [32][128] LDS tile (every
  // wave is past the last barrier, so the K/V/P images are dead) -> 16-B
  // row-major global stores.
  char* const ob = smem + wid * (QBLK * O_ROW);
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv = (l_run[qs][r] > 0.f) ? 1.0f / l_run[qs][r] : 0.f;
      char* orow = ob + (qs * 16 + lg * 4 + r) * O_ROW + l16 * 2;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
        *reinterpret_cast<short*>(orow + dt * 32) = f2bits(o[qs][dt][r] * inv);
    }
  }
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < QBLK / 4; ++i) {
    const int row = i * 4 + lg;
    const int qr = qtile * QBLK + row;
    if (qr < qlen)
      *reinterpret_cast<bf16x8*>(out + ((q_row0 + qr) * n_q + head) * D + l16 * 8) =
          *reinterpret_cast<const bf16x8*>(ob + row * O_ROW + l16 * 16);
  }
}

}  // namespace

void paged_prefill_attention(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             torch::Tensor page_table, torch::Tensor seq_lens,
                             torch::Tensor query_starts, torch::Tensor query_lens,
                             double scale, long max_qlen) {
  TORCH_CHECK(out.is_contiguous());
  TORCH_CHECK(q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
  const int n_q = q.size(1), Dh = q.size(2);
  const int n_kv = k_cache.size(1), PS = k_cache.size(3);
  const int B = seq_lens.size(0);
  const int max_pages = page_table.size(1);
  TORCH_CHECK(Dh == 128, "prefill attention: head_dim 128 only");
  TORCH_CHECK(n_q % 4 == 0, "n_q must be a multiple of 4");
  const int ratio = n_q / n_kv;
  TORCH_CHECK(ratio % 4 == 0 || ratio == n_q,
              "GQA ratio must be a multiple of 4 (waves of a workgroup share "
              "one kv head)");
  // 16-B vector access to q rows and out rows
  TORCH_CHECK(q.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "prefill attention: q rows and out must be 16-byte aligned");
  if (max_qlen <= 0) {
    // fallback: derive from the device tensor. This D2H copy BLOCKS the
    // host until the stream drains (measured ~2 ms/call under serving
    // load with a deep queue — 32x per prefill); hot callers pass
    // max_qlen explicitly (AttnMetadata.max_qlen).
    auto q_lens_cpu = query_lens.to(torch::kCPU);
    auto* ql = q_lens_cpu.data_ptr<int>();
    for (int i = 0; i < B; ++i)
      max_qlen = std::max<long>(max_qlen, ql[i]);
    if (max_qlen == 0) return;
  }
  const int qtiles = (max_qlen + QBLK - 1) / QBLK;
  TORCH_CHECK(B <= 65535 && qtiles <= 65535, "prefill attention: grid too large");
  int ps_shift = -1;
  if (PS > 0 && (PS & (PS - 1)) == 0)
    for (ps_shift = 0; (1 << ps_shift) < PS; ++ps_shift) {}
  auto stream = at::hip::getCurrentHIPStream();
#define PF_LAUNCH(CT, POW2)                                                    \
  hipLaunchKernelGGL((prefill_attn_kernel<CT, POW2>), dim3(n_q / 4, B, qtiles),\
                     dim3(256), 0, stream, (short*)out.data_ptr(),             \
                     (const short*)q.data_ptr(),                               \
                     (const CT*)k_cache.data_ptr(),                            \
                     (const CT*)v_cache.data_ptr(),                            \
                     page_table.data_ptr<int>(), seq_lens.data_ptr<int>(),     \
                     query_starts.data_ptr<int>(), query_lens.data_ptr<int>(), \
                     (float)scale, n_q, n_kv, PS, ps_shift, max_pages,         \
                     (long)q.stride(0))
  if (k_cache.scalar_type() == at::kFloat8_e4m3fn) {
    if (ps_shift >= 0) PF_LAUNCH(unsigned char, true);
    else PF_LAUNCH(unsigned char, false);
  } else {
    TORCH_CHECK(k_cache.scalar_type() == at::kBFloat16);
    if (ps_shift >= 0) PF_LAUNCH(short, true);
    else PF_LAUNCH(short, false);
  }
#undef PF_LAUNCH
}
