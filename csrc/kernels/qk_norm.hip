// Per-head QK-norm (Qwen3) + NeoX RoPE + paged KV-cache write, one launch after the plain QKV GEMM.
//
// qkv [T, (Hq + 2 Hkv) * 128] bf16 in natural column order [q | k | v] is read only. For each q / k
// head: n = x * rsqrt(mean(x^2) + eps) * gamma (q_norm for q heads, k_norm for k heads), then the
// NeoX rotation of (n_i, n_{i+64}) with cos_sin[positions[t]]; fp32 from the bf16 inputs to the one
// rounding at the bf16 store. q goes to q_out (the attention input), k to the paged K cache at
// slots[t], v unchanged to the V cache; slots[t] < 0 (a padded graph row) writes q only.
//
// Shape: 16 lanes per head, lane j owning elements 4j..4j+3 of each half (one 8-B load per half, the
// quads of rope_kv_kernel), so a head is one DPP row: the sum of squares is four row-local DPP adds
// (no LDS, no cross-row traffic) and the rotation partner is lane-local. A 256-thread block holds 16
// heads of one token; grid = T x ceil((Hq + Hkv) / 16), so no block loops and every load of a thread
// (row quads, cos / sin, gamma, its V vector) is requested before the first arithmetic. A head past
// Hq + Hkv re-reads the last head and a V vector past Hkv * 16 the last vector (loads stay
// unconditional, README "The compiler's waits"); only the stores are predicated.
// Plain vector loads and stores only: no atomics, no polls, no workspace.
#include "common.h"
#include "launchers.h"

namespace vgate {

template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// Sum over the 16 lanes of a DPP row; every lane of the row gets the same bits.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_row<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_row<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_row<0x141>(v);  // row_half_mirror: the other quad of the 8-lane half
  v += dpp_row<0x140>(v);  // row_mirror: the other half of the row
  return v;
}

__device__ __forceinline__ void unpack4(const uint2& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
}

__global__ __launch_bounds__(256) void qk_norm_rope_kv_kernel(const bf16_t* __restrict__ qkv,
                                                               const int32_t* __restrict__ positions,
                                                               const int32_t* __restrict__ slots,
                                                               const float* __restrict__ cos_sin,
                                                               const bf16_t* __restrict__ q_norm,
                                                               const bf16_t* __restrict__ k_norm, float eps,
                                                               bf16_t* __restrict__ k_cache,
                                                               bf16_t* __restrict__ v_cache, int Hq, int Hkv,
                                                               int BS, bf16_t* __restrict__ q_out, int ldq,
                                                               unsigned long long* tl) {
  TLScope tl_scope(tl);
  constexpr int D = 128, HALF = 64;
  const int t = blockIdx.x;
  const int nh = Hq + Hkv;
  const int h = blockIdx.y * 16 + (threadIdx.x >> 4);
  const int hh = min(h, nh - 1);
  const int i0 = (threadIdx.x & 15) * 4;
  const int nv = Hkv * (D / 8);  // 16-B vectors of the token's v heads
  const int vi = blockIdx.y * 256 + threadIdx.x;
  const bf16_t* row = qkv + (size_t)t * (nh + Hkv) * D;
  const int pos = positions[t];
  const int slot = slots ? slots[t] : -1;
  const float* cs = cos_sin + (size_t)pos * D;
  const bf16_t* base = row + hh * D;
  const bf16_t* gam = hh < Hq ? q_norm : k_norm;
  // every load first
  const uint2 a = *reinterpret_cast<const uint2*>(base + i0);
  const uint2 b = *reinterpret_cast<const uint2*>(base + HALF + i0);
  const uint2 ga = *reinterpret_cast<const uint2*>(gam + i0);
  const uint2 gb = *reinterpret_cast<const uint2*>(gam + HALF + i0);
  const float4 c = *reinterpret_cast<const float4*>(cs + i0);
  const float4 s = *reinterpret_cast<const float4*>(cs + HALF + i0);
  const uint4 vv = ld16(row + (size_t)nh * D + (size_t)min(vi, nv - 1) * 8);

  float x1[4], x2[4], g1[4], g2[4];
  unpack4(a, x1); unpack4(b, x2); unpack4(ga, g1); unpack4(gb, g2);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
  ss = row16_sum(ss);
  const float inv = rsqrtf(ss * (1.f / D) + eps);
  const float cc[4] = {c.x, c.y, c.z, c.w}, sn[4] = {s.x, s.y, s.z, s.w};
  float o1[4], o2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float n1 = x1[j] * inv * g1[j], n2 = x2[j] * inv * g2[j];
    o1[j] = n1 * cc[j] - n2 * sn[j];
    o2[j] = n2 * cc[j] + n1 * sn[j];
  }
  uint2 p1, p2;
  p1.x = pack_bf2(o1[0], o1[1]); p1.y = pack_bf2(o1[2], o1[3]);
  p2.x = pack_bf2(o2[0], o2[1]); p2.y = pack_bf2(o2[2], o2[3]);

  const int blk = slot >= 0 ? slot / BS : 0;
  const int off = slot >= 0 ? slot % BS : 0;
  if (h < Hq) {
    bf16_t* qd = q_out + (size_t)t * ldq + h * D;
    *reinterpret_cast<uint2*>(qd + i0) = p1;
    *reinterpret_cast<uint2*>(qd + HALF + i0) = p2;
  } else if (h < nh && slot >= 0) {
    bf16_t* dst = k_cache + (((size_t)blk * Hkv + (h - Hq)) * BS + off) * D;
    *reinterpret_cast<uint2*>(dst + i0) = p1;
    *reinterpret_cast<uint2*>(dst + HALF + i0) = p2;
  }
  if (vi < nv && slot >= 0) {
    bf16_t* dst = v_cache + (((size_t)blk * Hkv + (vi >> 4)) * BS + off) * D;
    *reinterpret_cast<uint4*>(dst + (vi & 15) * 8) = vv;
  }
}

void launch_qk_norm_rope_kv(const uint16_t* qkv, const int32_t* positions, const int32_t* slots,
                            const float* cos_sin, const uint16_t* q_norm, const uint16_t* k_norm, float eps,
                            uint16_t* k_cache, uint16_t* v_cache, int T, int Hq, int Hkv, int BS,
                            uint16_t* q_out, int ldq, hipStream_t st) {
  if (T <= 0) return;
  // 16 heads and 256 V vectors per block: ceil((Hq + Hkv) / 16) * 256 >= (Hq + Hkv) * 16 > Hkv * 16
  const int passes = (Hq + Hkv + 15) / 16;
  hipLaunchKernelGGL(qk_norm_rope_kv_kernel, dim3(T, passes), dim3(256), 0, st, qkv, positions, slots, cos_sin,
                     q_norm, k_norm, eps, k_cache, v_cache, Hq, Hkv, BS, q_out, ldq,
                     tl_take("qk_norm_rope_kv", T * passes));
}

}  // namespace vgate
