// Logits processors of the sampled rows, in place, before the sampler: repetition / frequency /
// presence penalties and logit_bias (vgate/runtime/logits_proc.py builds the per-step buffer).
//
// A row's history is a SPARSE list of unique-token entries {tok, cnt, bias, pad} (16 B; bit 31 of
// cnt = "token occurs in the prompt", low bits = occurrences in the output), so a step touches
// (entries) logits, not (vocab). Per token, in this order, each a separately rounded fp32 operation
// (vgate/ops/reference.py process_logits_ref is the dense oracle, compared bit for bit):
//   seen && rep != 1:  x = x > 0 ? x * inv_rep : x * rep
//                      x = x - freq * float(c)
//   c > 0:             x = x - pres
//                      x = x + bias
// Asynchronous scheduling: the sequence's newest output token may exist only in the previous step's
// sampler output (pend[row] = -(slot + 1), the convention of the step's token ids). The block reads
// it once (p = prev[slot]); the lane holding p's entry counts it, and when no entry holds it
// thread 0 applies the (seen, c = 1, bias = 0) update to logits[row, p] itself. The host keeps the
// tokens of a row unique, so no two lanes write one logit: no atomics. No spin, wait or hand-off
// word anywhere: every block does a bounded loop over its own row's entries and exits.
#include "common.h"
#include "launchers.h"

namespace vgate {

namespace {

constexpr int LP_BLOCK = 256;
constexpr int LP_UNROLL = 4;

struct LPPar {
  float rep, inv_rep, pres, freq;
};

// the four steps on one logit; contraction off: `x - freq * c` must stay a rounded product and a
// rounded difference. Plain operators inside this pragma's scope, not the __fmul_rn / __fsub_rn
// intrinsics: HIP defines those as plain operators in a header compiled with contraction allowed,
// so the compiler fuses them into v_fma_f32 once they are inlined here.
__device__ __forceinline__ float lp_apply(float x, int cnt, float bias, const LPPar& pr) {
#pragma clang fp contract(off)
  const int c = cnt & 0x7fffffff;
  const bool seen = cnt != 0;  // in-prompt bit or an output occurrence
  if (seen && pr.rep != 1.f) x = x > 0.f ? x * pr.inv_rep : x * pr.rep;
  const float fc = pr.freq * (float)c;
  x = x - fc;
  if (c > 0) x = x - pr.pres;
  return x + bias;
}

}  // namespace

__global__ __launch_bounds__(LP_BLOCK) void logits_process_kernel(
    float* __restrict__ logits, int ldl, int V, const int32_t* __restrict__ row_off, const int32_t* __restrict__ pend,
    const float* __restrict__ par, const uint4* __restrict__ ent, int nent, const int32_t* __restrict__ prev, int nprev,
    unsigned long long* tl) {
  TLScope tl_scope(tl);
  const int row = blockIdx.x;
  int beg = row_off[row], end = row_off[row + 1];
  const int pd = prev != nullptr ? pend[row] : 0;
  beg = max(beg, 0);
  end = min(end, nent);
  if (end <= beg && pd >= 0) return;  // block-uniform: nothing to do for this row
  int p = -1;  // the in-flight token of this row's sequence (block-uniform)
  if (pd < 0) {
    const int slot = min(max(-(pd + 1), 0), nprev - 1);
    p = prev[slot];
    if (p < 0 || p >= V) p = -1;
  }
  const float4 pv = *reinterpret_cast<const float4*>(par + 4 * (size_t)row);
  const LPPar pr{pv.x, pv.y, pv.z, pv.w};
  float* __restrict__ lrow = logits + (size_t)row * ldl;
  int matched = 0;
  for (int i0 = beg + (int)threadIdx.x; i0 < end; i0 += LP_BLOCK * LP_UNROLL) {
    uint4 e[LP_UNROLL];
    float x[LP_UNROLL];
    bool ok[LP_UNROLL];
    // entry loads, then the dependent logit gathers, then the stores
#pragma unroll
    for (int u = 0; u < LP_UNROLL; ++u) {
      const int i = i0 + u * LP_BLOCK;
      e[u] = i < end ? ld16(ent + i) : make_uint4(0xffffffffu, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < LP_UNROLL; ++u) {
      ok[u] = e[u].x < (uint32_t)V;  // also drops tok < 0 and the out-of-range filler above
      x[u] = ok[u] ? lrow[e[u].x] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < LP_UNROLL; ++u) {
      if (!ok[u]) continue;
      int cnt = (int)e[u].y;
      if ((int)e[u].x == p) {
        cnt += 1;
        matched = 1;
      }
      lrow[e[u].x] = lp_apply(x[u], cnt, __uint_as_float(e[u].z), pr);
    }
  }
  if (p >= 0) {  // block-uniform
    const int any = __syncthreads_or(matched);
    if (!any && threadIdx.x == 0) lrow[p] = lp_apply(lrow[p], 1, 0.f, pr);
  }
}

void launch_logits_process(float* logits, int ldl, int S, int V, const int32_t* row_off, const int32_t* pend,
                           const float* par, const void* ent, int nent, const int32_t* prev, int nprev,
                           hipStream_t st) {
  if (S <= 0 || V <= 0) return;
  hipLaunchKernelGGL(logits_process_kernel, dim3(S), dim3(LP_BLOCK), 0, st, logits, ldl, V, row_off, pend, par,
                     reinterpret_cast<const uint4*>(ent), nent, prev, nprev, tl_take("logits_process", S));
}

}  // namespace vgate
