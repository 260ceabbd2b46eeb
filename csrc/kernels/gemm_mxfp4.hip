// MXFP4 (OCP Microscaling: e2m1 codes, one e8m0 scale per 32 values along K) W4A16: the decode GEMM
// (M <= 16) and the mxfp4 -> bf16 scratch copy the prefill / mid / tile kernels read at M > 16.
//
// Packed codes Wq[N/16][K/128][64 lanes][16 B] (ops.pack_mxfp4): dword u (0..3) of lane l holds the eight
// e2m1 codes of W[16 nt + (l & 15)][128 kq + 32 u + 8 (l >> 4) + j], j = 0..7, code j in nibble j (low
// nibble of byte 0 first: the order of the conversion's byte select and pair output) — one 16-B lane load
// (1 KiB per wave, contiguous, non-temporal) is the A operand of four v_mfma_f32_16x16x32_bf16 k-steps.
// Rows are in the layout's permuted order (ops.row_permutation), as for the dense, AWQ and FP8 copies.
// Packed scales Sq[N/16][K/128][16 rows][4 B] (ops.pack_mxfp4_scales): byte u of row r is the e8m0 byte
// of the 32-block (row 16 nt + r, k-step 4 kq + u), so a lane's dword u lies in exactly one block and
// one 4-B load per 128-k unit (the same 64 B read by all four lane groups) carries its four scales.
//
// A weight is value(code) * 2^(e - 127): exact in bf16 for 2 <= e <= 252 (2 significant bits; 0.5 * 2^-125
// is normal, 6 * 2^125 finite), which is what the Linear admits. The scale goes INTO the conversion
// (v_cvt_scalef32_pk_bf16_fp4 through the compiler's builtin, conversion scale bitcast(e << 23), a power
// of two: exact whether the instruction multiplies or adds exponents), so the hazard recognizer sees the
// producer of every MFMA operand and no scale ever touches an accumulator.
#include "gemm_decode.h"

namespace vgate {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 8 e2m1 codes (one dword, code j in nibble j) times 2^(e - 127) -> the bf16 MFMA fragment, exact
__device__ __forceinline__ bf16x8 fp4x8_bf16(uint32_t q, uint32_t e) {
  const float s = __uint_as_float(e << 23);
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 3);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// Shaped like fp8_gemm_kernel (gemm_fp8.hip): grid = (tile groups, 1, K slices); the waves of a block
// split the slice's k-range in units of 128 k. Chunks of QC units: EVERY load of a chunk (fp4 fragments,
// scale dwords, activations, gamma) is issued before the first is consumed. Rows >= M are zero and never
// loaded; a clamped re-load past the range end is in bounds and never consumed. NORM 1: gamma in
// registers + the deferred row scale (gemm_finish), as the FP8 and AWQ kernels'. NTB tiles per block
// share the block's activation fragments (loads, x^2 and gamma work): at 4 bits a one-tile block issues
// one weight load per 128 k against 4 activation + 4 gamma loads.
template <int NTB, int EPI, int NORM>
__global__ __launch_bounds__(512) void mxfp4_gemm_kernel(GemmParams p) {
  static_assert(NORM == 0 || NORM == 1, "mxfp4 decode: no norm, or gamma in registers");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TLScope tl_scope(p.dbg_ts);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int KQ = p.K >> 7;  // units of 128 k
  const int nt0 = blockIdx.x * NTB;
  const int s0 = (KQ * blockIdx.z) / p.splitk, s1 = (KQ * (blockIdx.z + 1)) / p.splitk;
  const int qbeg = s0 + ((s1 - s0) * wid) / nw;
  const int qend = s0 + ((s1 - s0) * (wid + 1)) / nw;
  const uint32_t* sq = reinterpret_cast<const uint32_t*>(p.scales) + (lane & 15);  // Sq (launch_mxfp4_gemm)
  f32x4 acc[1][NTB];
#pragma unroll
  for (int b = 0; b < NTB; ++b) acc[0][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int m = lane & 15;
  const bool xok = m < p.M;
  const bf16_t* xrow = p.x + (size_t)(xok ? m : p.M - 1) * p.lda + 8 * (lane >> 4);
  float ssr[1] = {0.f};
  const bf16_t* nw_ptr = p.norm_w ? p.norm_w + 8 * (lane >> 4) : nullptr;
  constexpr int QC = NTB == 4 ? 2 : 4;  // (4 tiles: half the chunk for the registers)
  for (int kc = qbeg; kc < qend; kc += QC) {
    uint4 w[QC][NTB];
    uint32_t sc[QC][NTB];
    uint4 a[QC][4];
    uint4 gm[QC][4];
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      const int kq = min(kc + c, qend - 1);  // clamped re-load past the end: never consumed
#pragma unroll
      for (int j = 0; j < NTB; ++j) {
        const size_t unit = (size_t)(nt0 + j) * KQ + kq;
        w[c][j] = ld_nt16(p.wp + unit * 64 + lane);
        sc[c][j] = sq[unit * 16];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[c][u] = xok ? *reinterpret_cast<const uint4*>(xrow + (kq * 4 + u) * 32) : make_uint4(0, 0, 0, 0);
        if constexpr (NORM == 1) gm[c][u] = *reinterpret_cast<const uint4*>(nw_ptr + (kq * 4 + u) * 32);
      }
    }
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      if (kc + c >= qend) break;  // wave-uniform
      if constexpr (NORM == 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float f[8], g[8];
          unpack8(a[c][u], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ssr[0] += f[j] * f[j];
          unpack8(gm[c][u], g);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] *= g[j];
          a[c][u] = pack8(f);
        }
      }
#pragma unroll
      for (int j = 0; j < NTB; ++j) {
        const uint4 q = w[c][j];
        const uint32_t e = sc[c][j];
        const bf16x8 wf[4] = {fp4x8_bf16(q.x, e & 0xFF), fp4x8_bf16(q.y, (e >> 8) & 0xFF),
                              fp4x8_bf16(q.z, (e >> 16) & 0xFF), fp4x8_bf16(q.w, e >> 24)};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[0][j] = mfma16(wf[u], as_bf16x8(a[c][u]), acc[0][j]);
      }
    }
  }
  gemm_finish<1, NTB, EPI, NORM, false>(p, acc, ssr, smem, 0, nt0, EpiPre<NTB>{});
}

// ---- mxfp4 prefill operand: e2m1 fragments -> bf16 fragments (the dense fragment order) ----
// Steps of M > 16 rows run the bf16 prefill / mid / tile kernels on a per-call scratch copy of ONE
// matrix, the counterpart of fp8_dequant_packed_kernel: each element is bf16(value * 2^(e-127) * gamma);
// the scaled conversion is exact in bf16, so without gamma nothing rounds and with it the fp32 product
// rounds once. One thread per (tile, 128-k unit, lane): 16 B + 4 B in, 4 x 16 B out.
__global__ __launch_bounds__(256) void mxfp4_dequant_packed_kernel(const uint4* __restrict__ wq,
                                                                   const uint32_t* __restrict__ sq,
                                                                   const bf16_t* __restrict__ gamma,
                                                                   uint4* __restrict__ out, int N, int K) {
  const int KQ = K >> 7;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // ((nt * KQ) + kq) * 64 + lane
  if (idx >= (size_t)(N >> 4) * KQ * 64) return;
  const int lane = (int)(idx & 63);
  const size_t unit = idx >> 6;
  const int kq = (int)(unit % KQ);
  const size_t nt = unit / KQ;
  const uint4 q = wq[idx];
  const uint32_t e = sq[unit * 16 + (lane & 15)];
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bf16x8 v = fp4x8_bf16(qw[u], (e >> (8 * u)) & 0xFF);
    uint4 o = *reinterpret_cast<const uint4*>(&v);
    if (gamma != nullptr) {
      const int k0 = (kq * 4 + u) * 32 + 8 * (lane >> 4);
      float f[8], g8[8];
      unpack8(o, f);
      unpack8(*reinterpret_cast<const uint4*>(gamma + k0), g8);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] *= g8[j];
      o = pack8(f);
    }
    out[((nt * (K >> 5)) + kq * 4 + u) * 64 + lane] = o;
  }
}

void launch_mxfp4_dequant(const void* wq, const void* sq, const uint16_t* gamma, void* out, int N, int K,
                          hipStream_t st) {
  const size_t n = (size_t)(N / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(mxfp4_dequant_packed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(wq), reinterpret_cast<const uint32_t*>(sq),
                     reinterpret_cast<const bf16_t*>(gamma), reinterpret_cast<uint4*>(out), N, K);
}

template <int NTB, int EPI, int NORM>
static void mxfp4_launch(GemmParams p, const GemmArgs& g, hipStream_t st) {
  const int nblk = g.N / 16 / NTB;
  const int KQ = g.K / 128;
  Plan pl = plan(nblk, 1, KQ, 1, NTB, g.waves, g.splitk);
  if (pl.waves > 8) pl.waves = 8;  // __launch_bounds__(512)
  const size_t need_slab = (size_t)nblk * pl.splitk * (NTB * 64 * 16 + (NORM ? 16 * 4 : 0));
  if (pl.splitk > 1 && (g.slabs == nullptr || need_slab > g.slab_bytes || nblk > g.max_counters))
    pl.splitk = 1;  // workspace too small: one slice (still correct)
  p.splitk = pl.splitk;
  // two slices meet through granules, more through slabs + ticket (launch_one, gemm_decode.h)
  const size_t need_g = (size_t)nblk * (2 * NTB + 1) * 64 * 16;
  if (NTB == 1 && pl.splitk == 2 && g.sk_pub != nullptr && need_g <= g.sk_bytes)
    p.gran = reinterpret_cast<uint4*>(g.sk_pub);
  const size_t lds = red_bytes<1, NTB>(pl.waves) + ssq_bytes<1>(pl.waves) + 16;
  dim3 grid(nblk, 1, pl.splitk), block(64 * pl.waves);
  if (p.dbg_ts == nullptr) p.dbg_ts = tl_take("mxfp4_gemm", (int)(grid.x * grid.z));
  hipLaunchKernelGGL((mxfp4_gemm_kernel<NTB, EPI, NORM>), grid, block, lds, st, p);
}

// Tiles per block when the caller forces none (benchmarks/probes/mxfp4_sweep.py --ntb 1,2,4, cold weights, M = 8,
// profiles/mxfp4_sweep_ntb.log): four from 1024 tiles up — gate_up, Llama-3-8B (1792 tiles) 44.0 -> 31.0 (two) ->
// 25.5 us (four), Qwen2.5-1.5B (1120 tiles) 18.5 -> 15.4 -> 14.6 us — and one below, where groups leave CUs idle
// (Llama-3-8B o, 256 tiles: 9.3 -> 10.1 -> 12.2 us; down 17.5 -> 19.3 -> 24.1 us; the 96-tile Qwen o / down
// likewise). Nothing between 256 and 1120 tiles was measured: the threshold is the FP8 rule's. qkv keeps one tile
// per block by its layout.
static int mxfp4_ntb_rule(int ntiles) { return ntiles >= 1024 ? 4 : 1; }

bool launch_mxfp4_gemm(const GemmArgs& g, hipStream_t st) {
  if (g.M <= 0 || g.M > 16 || g.mxfp4_scales == nullptr || g.N % 16 != 0 || g.K % 128 != 0 ||
      g.row_idx != nullptr || g.rownorm || g.ar_world > 0 || g.fa != nullptr || g.ssp_in != nullptr ||
      g.ssp_out != nullptr || g.hg != nullptr)
    return false;
  GemmParams p = gemm_params(g);
  p.scales = reinterpret_cast<const bf16_t*>(g.mxfp4_scales);  // the kernel reads them as Sq dwords
  // tiles per block: g.ntb 1 / 2 / 4 forced (a count the tiles do not divide into: one tile), else mxfp4_ntb_rule
  const int ntiles = g.N / 16;
  int ntb = g.ntb == 2 || g.ntb == 4 ? g.ntb : g.ntb == 1 ? 1 : mxfp4_ntb_rule(ntiles);
  if (g.epi == EPI_QKV || ntiles % ntb != 0) ntb = 1;  // (QKV tiles carry their rotation partners: one per block)
  with_epi(g.epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    auto go = [&](auto nt) {
      constexpr int NTB = decltype(nt)::value;
      if (g.norm_w != nullptr) mxfp4_launch<NTB, EPI, 1>(p, g, st);
      else mxfp4_launch<NTB, EPI, 0>(p, g, st);
    };
    if constexpr (EPI != EPI_QKV) {
      if (ntb == 4) return go(std::integral_constant<int, 4>{});
      if (ntb == 2) return go(std::integral_constant<int, 2>{});
    }
    go(std::integral_constant<int, 1>{});
  });
  return true;
}

}  // namespace vgate
