// FP8 (OCP e4m3fn) W8A16: the decode GEMM (M <= 16) and the fp8 -> bf16 scratch copy the prefill /
// mid / tile kernels read at M > 16.
//
// Packed operand Wq[N/16][K/64][64 lanes][16 B] (ops.pack_fp8): byte 8u + j of lane l is the e4m3fn
// code of W[16 nt + (l & 15)][64 kp + 32 u + 8 (l >> 4) + j], u = 0, 1, j = 0..7 — one 16-B lane load
// (1 KiB per wave, contiguous, non-temporal) is the A operand of two v_mfma_f32_16x16x32_bf16
// k-steps. Rows are in the layout's permuted order (ops.row_permutation), as for the dense and AWQ
// copies. Scales: fp32 [G][N] in the same row order, G = 1 (per channel) or K / 128 (block scales); a
// lane's accumulator holds D[n = 4 (l >> 4) + i][m = l & 15], so its four scales of a (tile, group)
// are one 16-B load.
//
// e4m3 -> bf16 is exact (4 significant bits, exponents 2^-9 .. 2^8), so the codes are converted in
// registers (v_cvt_scalef32_pk_bf16_fp8 through the compiler's builtin, conversion scale 1.0: the
// hazard recognizer sees the producer of every MFMA operand) and the scales are applied in fp32 to
// ACCUMULATORS, never to weights: the decode result carries no per-weight rounding.
#include "gemm_decode.h"

namespace vgate {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn codes (two dwords, element j in byte j) -> the bf16 MFMA fragment, exact
__device__ __forceinline__ bf16x8 fp8x8_bf16(uint32_t lo, uint32_t hi) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// Shaped like awq_gemm_kernel (gemm_decode.h): grid = (tile groups, 1, K slices); the waves of a
// block split the slice's k-range in units of 128 k (two packed k-pairs), so a scale group never
// straddles a wave or a slice. Chunks of QC units: EVERY load of a chunk (fp8 fragments,
// activations, gamma, scales) is issued before the first is consumed. Rows >= M are zero and never
// loaded; a clamped re-load past the range end is in bounds and never consumed.
// GROUPED: each 128-k group accumulates into a temporary folded in as acc += s * tmp; otherwise the
// per-channel scale is applied once, before gemm_finish. NORM 1: gamma in registers + the deferred
// row scale (gemm_finish), as the AWQ kernel's. NTB tiles per block share the block's activation
// fragments (loads, x^2 and gamma work): with one-byte weights these are most of what a one-tile block
// issues (per 128 k: 2 weight loads against 4 activation + 4 gamma loads).
template <int NTB, int EPI, int NORM, bool GROUPED>
__global__ __launch_bounds__(512) void fp8_gemm_kernel(GemmParams p) {
  static_assert(NORM == 0 || NORM == 1, "fp8 decode: no norm, or gamma in registers");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TLScope tl_scope(p.dbg_ts);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int KQ = p.K >> 7;  // units of 128 k
  const int nt0 = blockIdx.x * NTB;
  const int s0 = (KQ * blockIdx.z) / p.splitk, s1 = (KQ * (blockIdx.z + 1)) / p.splitk;
  const int qbeg = s0 + ((s1 - s0) * wid) / nw;
  const int qend = s0 + ((s1 - s0) * (wid + 1)) / nw;
  const float* fsc = reinterpret_cast<const float*>(p.scales);  // fp32 [G][N] (launch_fp8_gemm)
  f32x4 acc[1][NTB];
#pragma unroll
  for (int b = 0; b < NTB; ++b) acc[0][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int m = lane & 15;
  const bool xok = m < p.M;
  const bf16_t* xrow = p.x + (size_t)(xok ? m : p.M - 1) * p.lda + 8 * (lane >> 4);
  float ssr[1] = {0.f};
  const bf16_t* nw_ptr = p.norm_w ? p.norm_w + 8 * (lane >> 4) : nullptr;
  const float* sc_ptr = fsc + 4 * (lane >> 4);  // + group * N + tile * 16: this lane's 4 output columns
  f32x4 pcs[NTB];  // per-channel scales: requested ahead of the stream, applied after it
  if constexpr (!GROUPED) {
#pragma unroll
    for (int j = 0; j < NTB; ++j) pcs[j] = *reinterpret_cast<const f32x4*>(sc_ptr + (nt0 + j) * 16);
  }
  constexpr int QC = NTB == 4 ? 2 : 4;  // (4 tiles: 8 weight fragments per unit, half the chunk for the registers)
  for (int kc = qbeg; kc < qend; kc += QC) {
    uint4 w[QC][2][NTB];
    uint4 a[QC][4];
    uint4 gm[QC][4];
    f32x4 sc[QC][NTB];
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      const int kq = min(kc + c, qend - 1);  // clamped re-load past the end: never consumed
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < NTB; ++j) w[c][h][j] = ld_nt16(p.wp + ((size_t)(nt0 + j) * (2 * KQ) + 2 * kq + h) * 64 + lane);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[c][u] = xok ? *reinterpret_cast<const uint4*>(xrow + (kq * 4 + u) * 32) : make_uint4(0, 0, 0, 0);
        if constexpr (NORM == 1) gm[c][u] = *reinterpret_cast<const uint4*>(nw_ptr + (kq * 4 + u) * 32);
      }
      if constexpr (GROUPED) {
#pragma unroll
        for (int j = 0; j < NTB; ++j)
          sc[c][j] = *reinterpret_cast<const f32x4*>(sc_ptr + (size_t)kq * p.N + (nt0 + j) * 16);
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
        const uint4 w0 = w[c][0][j], w1 = w[c][1][j];
        const bf16x8 wf[4] = {fp8x8_bf16(w0.x, w0.y), fp8x8_bf16(w0.z, w0.w), fp8x8_bf16(w1.x, w1.y),
                              fp8x8_bf16(w1.z, w1.w)};
        if constexpr (GROUPED) {
          f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int u = 0; u < 4; ++u) t = mfma16(wf[u], as_bf16x8(a[c][u]), t);
          acc[0][j] += sc[c][j] * t;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[0][j] = mfma16(wf[u], as_bf16x8(a[c][u]), acc[0][j]);
        }
      }
    }
  }
  if constexpr (!GROUPED) {  // per-channel scale, once per wave partial (linear: the waves' and slices' sums follow)
#pragma unroll
    for (int j = 0; j < NTB; ++j) acc[0][j] *= pcs[j];
  }
  gemm_finish<1, NTB, EPI, NORM, false>(p, acc, ssr, smem, 0, nt0, EpiPre<NTB>{});
}

// ---- fp8 prefill operand: e4m3 fragments -> bf16 fragments (the dense fragment order) ----
// Steps of M > 16 rows run the bf16 prefill / mid / tile kernels on a per-call scratch copy of ONE
// matrix, the counterpart of awq_dequant_packed_kernel: each element is bf16(fp32(code) * s * gamma).
// One thread per (tile, k-pair, lane): 16 B in, 2 x 16 B out.
__global__ __launch_bounds__(256) void fp8_dequant_packed_kernel(const uint4* __restrict__ wq,
                                                                 const float* __restrict__ scales,
                                                                 const bf16_t* __restrict__ gamma,
                                                                 uint4* __restrict__ out, int N, int K, int groups) {
  const int KP = K >> 6;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // ((nt * KP) + kp) * 64 + lane
  if (idx >= (size_t)(N >> 4) * KP * 64) return;
  const int lane = (int)(idx & 63);
  const size_t tp = idx >> 6;
  const int kp = (int)(tp % KP), nt = (int)(tp / KP);
  const int n = nt * 16 + (lane & 15);
  const float s = scales[(size_t)(groups > 1 ? kp >> 1 : 0) * N + n];
  const uint4 q = wq[idx];
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int k0 = (kp * 2 + u) * 32 + 8 * (lane >> 4);
    float f[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(qw[2 * u + h], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(qw[2 * u + h], true);
      f[4 * h + 0] = lo[0] * s; f[4 * h + 1] = lo[1] * s;
      f[4 * h + 2] = hi[0] * s; f[4 * h + 3] = hi[1] * s;
    }
    if (gamma != nullptr) {
      float g8[8];
      unpack8(*reinterpret_cast<const uint4*>(gamma + k0), g8);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] *= g8[j];
    }
    out[(((size_t)nt * (K >> 5)) + kp * 2 + u) * 64 + lane] = pack8(f);
  }
}

void launch_fp8_dequant(const void* wq, const float* scales, int groups, const uint16_t* gamma, void* out, int N,
                        int K, hipStream_t st) {
  const size_t n = (size_t)(N / 16) * (K / 64) * 64;
  hipLaunchKernelGGL(fp8_dequant_packed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(wq), scales, reinterpret_cast<const bf16_t*>(gamma),
                     reinterpret_cast<uint4*>(out), N, K, groups);
}

template <int NTB, int EPI, int NORM, bool GROUPED>
static void fp8_launch(GemmParams p, const GemmArgs& g, hipStream_t st) {
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
  if (p.dbg_ts == nullptr) p.dbg_ts = tl_take("fp8_gemm", (int)(grid.x * grid.z));
  hipLaunchKernelGGL((fp8_gemm_kernel<NTB, EPI, NORM, GROUPED>), grid, block, lds, st, p);
}

// Tiles per block when the caller forces none (benchmarks/probes/fp8_sweep.py --fp8-ntb, cold weights, M = 8,
// profiles/fp8_sweep_ntb.log): two from 1024 tiles up — gate_up, Llama-3-8B 45.7 -> 33.4 us, Qwen2.5-1.5B 18.7 ->
// 16.1 us (four: 38.0 / 16.5) — and one below, where pairs leave CUs idle (Llama-3-8B down 19.3 -> 23.9 us,
// o 9.7 -> 10.8; qkv keeps one tile per block by its layout)
static int fp8_ntb_rule(int ntiles) { return ntiles >= 1024 ? 2 : 1; }

bool launch_fp8_gemm(const GemmArgs& g, hipStream_t st) {
  if (g.M <= 0 || g.M > 16 || g.fp8_scales == nullptr || g.N % 16 != 0 || g.K % 128 != 0 ||
      (g.fp8_groups != 1 && g.fp8_groups != g.K / 128) || g.row_idx != nullptr || g.rownorm || g.ar_world > 0 ||
      g.fa != nullptr || g.ssp_in != nullptr || g.ssp_out != nullptr || g.hg != nullptr)
    return false;
  GemmParams p = gemm_params(g);
  p.scales = reinterpret_cast<const bf16_t*>(g.fp8_scales);  // the kernel reads them as fp32 [G][N]
  const bool grouped = g.fp8_groups > 1;
  // tiles per block: g.ntb 1 / 2 / 4 forced (a count the tiles do not divide into: one tile), else FP8_NTB_RULE
  const int ntiles = g.N / 16;
  int ntb = g.ntb == 2 || g.ntb == 4 ? g.ntb : g.ntb == 1 ? 1 : fp8_ntb_rule(ntiles);
  if (g.epi == EPI_QKV || ntiles % ntb != 0) ntb = 1;  // (QKV tiles carry their rotation partners: one per block)
  with_epi(g.epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    auto go = [&](auto nt) {
      constexpr int NTB = decltype(nt)::value;
      if (g.norm_w != nullptr) {
        if (grouped) fp8_launch<NTB, EPI, 1, true>(p, g, st);
        else fp8_launch<NTB, EPI, 1, false>(p, g, st);
      } else {
        if (grouped) fp8_launch<NTB, EPI, 0, true>(p, g, st);
        else fp8_launch<NTB, EPI, 0, false>(p, g, st);
      }
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
