// Per-token log-probabilities of the sampled rows on gfx950: the chosen token's log-softmax and the
// row's k <= 20 most likely tokens with theirs, over the full vocabulary (V ~ 128k-152k).
//
// The distribution is the softmax at temperature 1 of the logits row exactly as the sampler read it
// (after penalties and logit_bias, before temperature / top-k / top-p), so these launches run after
// the sampler on the step's logits buffer, and the chosen token is the sampler's output.
// Ranking: raw fp32 logit descending, ties to the lower token id — a total order, exact in fp32.
// A -inf logit has log-probability -inf and ranks last. NaN logits are out of contract.
//
// Two plain launches, no in-launch hand-off: every block does bounded work and exits (no spin,
// poll, ticket, atomic or fault-word bit anywhere).
//   logprob_part_kernel   grid (NSEG, S): a block sweeps its contiguous slice of the row once, in
//     chunks of 5 float4 per thread held in registers (one chunk at V = 152k / 32 segments), and
//     keeps the slice's online (max, sum 2^((x - max) log2e)) and, per wave, a sorted list of the
//     best k entries across the wave's lanes, each (value, id) packed into one 64-bit key whose
//     unsigned order is the ranking: repeated wave maximum over DPP / permlane exchanges (lane_x),
//     each round taking the largest key strictly below the previous winner; a later chunk that holds
//     no key above the list's k-th costs one ballot. Wave 0 then merges the four lists and the four
//     (max, sum) pairs and writes the partial {m, l, 20 x (value, id)} with plain 8-B vector stores.
//   logprob_merge_kernel  one wave per row: merges the row's partials in fixed segment order
//     (bit-reproducible), selects the k best of the segments' lists the same way and writes the
//     row's record.
// Nothing at or beyond column V is read: a trailing float4 that straddles V is loaded by scalars.
#include "launchers.h"
#include "sampling_common.h"

namespace vgate {

namespace {

constexpr int LPB_THREADS = 256;
constexpr int LPB_WAVES = LPB_THREADS / 64;
constexpr int LPB_U = 5;            // float4 loads in flight per thread = one chunk
constexpr int LPB_E = 4 * LPB_U;    // elements per thread per chunk
constexpr int LPB_NONE = 0x7fffffff;  // id of "no entry" in a partial
constexpr int LPM_N = LOGPROB_SEGS * LOGPROB_TOP / 64;  // merge kernel: candidates per lane

// The ranking as one unsigned 64-bit key, larger = earlier: the fp32 value mapped monotonically to
// 32 bits (x + 0.0f first, so -0.0 and 0.0 tie) above the complemented id (ties go to the lower id).
// Keys of real entries are unique and non-zero; LPK_NONE = 0 is "no candidate" and loses to all.
typedef unsigned long long lpkey;
constexpr lpkey LPK_NONE = 0ull;

__device__ __forceinline__ lpkey lp_key(float v, int id) {
  const uint32_t b = __float_as_uint(v + 0.0f);
  const uint32_t u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((lpkey)u << 32) | (uint32_t)~id;
}
__device__ __forceinline__ float lp_key_value(lpkey k) {
  const uint32_t u = (uint32_t)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ int lp_key_id(lpkey k) { return (int)~(uint32_t)k; }

template <int K>
__device__ __forceinline__ void key_step(lpkey& k) {
  const uint32_t lo = lane_x<K>((uint32_t)k), hi = lane_x<K>((uint32_t)(k >> 32));
  const lpkey o = ((lpkey)hi << 32) | lo;
  k = o > k ? o : k;
}

// wave maximum of the keys, as a wave-uniform value (every lane ends with it: max is exact)
__device__ __forceinline__ lpkey wave_best(lpkey k) {
  key_step<1>(k);
  key_step<2>(k);
  key_step<4>(k);
  key_step<8>(k);
  key_step<16>(k);
  key_step<32>(k);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)k), hi = __builtin_amdgcn_readfirstlane((uint32_t)(k >> 32));
  return ((lpkey)hi << 32) | lo;
}

__device__ __forceinline__ lpkey key_of_lane(lpkey k, int lane_uniform) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)k, lane_uniform);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(k >> 32), lane_uniform);
  return ((lpkey)hi << 32) | lo;
}

template <int K>
__device__ __forceinline__ float max_step(float v) {
  return fmaxf(v, __uint_as_float(lane_x<K>(__float_as_uint(v))));
}
template <int K>
__device__ __forceinline__ float add_step(float v) {
  return v + __uint_as_float(lane_x<K>(__float_as_uint(v)));
}
// wave maximum, the same bits in every lane
__device__ __forceinline__ float wave_max(float v) {
  return max_step<32>(max_step<16>(max_step<8>(max_step<4>(max_step<2>(max_step<1>(v))))));
}
// wave sum by a fixed tree (lane 0's association order is what the callers use)
__device__ __forceinline__ float wave_sum(float v) {
  return add_step<32>(add_step<16>(add_step<8>(add_step<4>(add_step<2>(add_step<1>(v))))));
}
// l rescaled from its own maximum m to the common maximum M >= m
__device__ __forceinline__ float ml_rescale(float m, float l, float M) {
  return m == -INFINITY ? 0.f : l * exp2f((m - M) * LOG2E_S);
}

// (m, l) + (om, ol), this one first: the fixed-order merges of waves and segments
__device__ __forceinline__ void ml_merge(float& m, float& l, float om, float ol) {
  const float nm = fmaxf(m, om);
  l = (m == -INFINITY ? 0.f : l * exp2f((m - nm) * LOG2E_S)) + (om == -INFINITY ? 0.f : ol * exp2f((om - nm) * LOG2E_S));
  m = nm;
}

// The wave's sorted list lives across its lanes: lane j < kk holds the key of the j-th best seen so
// far (LPK_NONE: none yet). Merge this wave's N candidates per lane into it, exact: when no candidate
// beats the list's kk-th entry the list stands (one ballot: what a later chunk of a long row costs);
// otherwise round r takes the largest key strictly below round r - 1's winner among the candidates
// and the old list alike (keys are unique, so nothing is marked or removed) and lane r keeps it.
// kk (1..20) must be wave-uniform; the control flow is wave-uniform throughout.
template <int N>
__device__ __forceinline__ void wave_select(const lpkey (&ek)[N], lpkey& list, int lane, int kk) {
  const lpkey thr = key_of_lane(list, kk - 1);
  bool any = false;
#pragma unroll
  for (int u = 0; u < N; ++u) any |= ek[u] > thr;
  if (__ballot(any) == 0ull) return;
  lpkey last = ~0ull, fresh = LPK_NONE;
  for (int it = 0; it < kk; ++it) {
    lpkey best = list < last ? list : LPK_NONE;
#pragma unroll
    for (int u = 0; u < N; ++u) best = (ek[u] < last && ek[u] > best) ? ek[u] : best;
    const lpkey w = wave_best(best);
    if (w == LPK_NONE) break;  // fewer than kk entries in all
    fresh = lane == it ? w : fresh;
    last = w;
  }
  list = fresh;
}

}  // namespace

__global__ __launch_bounds__(LPB_THREADS) void logprob_part_kernel(LogprobArgs a, unsigned long long* tl) {
  TLScope tl_scope(tl);
  __shared__ lpkey s_k[LPB_WAVES][LOGPROB_TOP];
  __shared__ float s_m[LPB_WAVES], s_l[LPB_WAVES];
  const int seg = blockIdx.x, nseg = gridDim.x, row = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int kr = a.k_rows[row];
  if (kr < 0) return;  // block-uniform: the row did not ask
  const int kk = __builtin_amdgcn_readfirstlane(min(kr, LOGPROB_TOP));
  const int V = a.V;
  const int V4 = (V + 3) >> 2;  // float4 pieces, the last one may straddle V
  const int v_lo = (int)(((long long)V4 * seg) / nseg), v_hi = (int)(((long long)V4 * (seg + 1)) / nseg);
  const float* x = a.logits + (size_t)row * a.ldl;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float m = -INFINITY, l = 0.f;  // this thread's online (max, sum) over its elements
  lpkey list = LPK_NONE;         // the wave's list, lane j = j-th best
  for (int c0 = v_lo; c0 < v_hi; c0 += LPB_THREADS * LPB_U) {
    float4 q[LPB_U];
    // lanes past the slice load nothing; the float4 that straddles V is read by in-range scalars
#pragma unroll
    for (int u = 0; u < LPB_U; ++u) {
      const int vi = c0 + u * LPB_THREADS + tid;
      q[u] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (vi < v_hi) {
        if (4 * vi + 3 < V) {
          q[u] = x4[vi];
        } else {
          if (4 * vi < V) q[u].x = x[4 * vi];
          if (4 * vi + 1 < V) q[u].y = x[4 * vi + 1];
          if (4 * vi + 2 < V) q[u].z = x[4 * vi + 2];
        }
      }
    }
    float ev[LPB_E];
    lpkey ek[LPB_E];
    float cm = -INFINITY;
#pragma unroll
    for (int u = 0; u < LPB_U; ++u) {
      const int vi = c0 + u * LPB_THREADS + tid;
      const float e[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int id = 4 * vi + j;
        ev[4 * u + j] = e[j];
        ek[4 * u + j] = (vi < v_hi && id < V) ? lp_key(e[j], id) : LPK_NONE;
        cm = fmaxf(cm, e[j]);
      }
    }
    if (cm > -INFINITY) {  // (a chunk of -inf only adds nothing)
      const float nm = fmaxf(m, cm);
      float cs = 0.f;
#pragma unroll
      for (int u = 0; u < LPB_E; ++u) cs += exp2f((ev[u] - nm) * LOG2E_S);  // -inf (also the fillers) -> 0
      l = (m == -INFINITY ? 0.f : l * exp2f((m - nm) * LOG2E_S)) + cs;
      m = nm;
    }
    if (kk > 0) wave_select<LPB_E>(ek, list, lane, kk);
  }
  // the wave's (max, sum): one rescale per lane to the wave maximum, then a fixed 6-level tree
  const float wm = wave_max(m);
  const float wl = wave_sum(ml_rescale(m, l, wm));
  if (lane == 0) {
    s_m[wid] = wm;
    s_l[wid] = wl;
  }
  if (lane < LOGPROB_TOP) s_k[wid][lane] = list;  // (LPK_NONE from lane kk on)
  __syncthreads();
  if (wid != 0) return;
  // wave 0: the four waves' lists (80 candidates, two per lane) and (m, l) in wave order
  lpkey ck[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = lane + 64 * u;
    ck[u] = c < LPB_WAVES * LOGPROB_TOP ? s_k[c / LOGPROB_TOP][c % LOGPROB_TOP] : LPK_NONE;
  }
  lpkey best = LPK_NONE;
  if (kk > 0) wave_select<2>(ck, best, lane, kk);
  float bm = s_m[0], bl = s_l[0];
#pragma unroll
  for (int w = 1; w < LPB_WAVES; ++w) ml_merge(bm, bl, s_m[w], s_l[w]);
  // partial: words 0, 1 = (m, l), words 2 + 2 j, 3 + 2 j = (value, id) of entry j, (-inf, LPB_NONE) = none
  float* part = a.part + ((size_t)row * LOGPROB_SEGS + seg) * LOGPROB_PART_WORDS;
  if (lane == 0) reinterpret_cast<float2*>(part)[0] = make_float2(bm, bl);
  if (lane < LOGPROB_TOP) {
    const bool ok = best != LPK_NONE;
    reinterpret_cast<float2*>(part)[1 + lane] =
        make_float2(ok ? lp_key_value(best) : -INFINITY, __int_as_float(ok ? lp_key_id(best) : LPB_NONE));
  }
}

__global__ __launch_bounds__(64) void logprob_merge_kernel(LogprobArgs a, int nseg, unsigned long long* tl) {
  TLScope tl_scope(tl);
  const int row = blockIdx.x, lane = threadIdx.x;
  const int kr = a.k_rows[row];
  if (kr < 0) return;  // block-uniform
  const int kk = __builtin_amdgcn_readfirstlane(min(kr, LOGPROB_TOP));
  const float* part = a.part + (size_t)row * LOGPROB_SEGS * LOGPROB_PART_WORDS;
  // every load up front (they do not depend on one another): the chosen token and its logit, the
  // segments' (m, l) and the lane's candidates
  const int tok = min(max(a.tokens[row], 0), a.V - 1);
  const float xt = a.logits[(size_t)row * a.ldl + tok];
  float2 ml = make_float2(-INFINITY, 0.f);
  if (lane < nseg) ml = *reinterpret_cast<const float2*>(part + (size_t)lane * LOGPROB_PART_WORDS);
  lpkey ck[LPM_N];
#pragma unroll
  for (int u = 0; u < LPM_N; ++u) {
    const int c = lane + 64 * u, s = c / LOGPROB_TOP, j = c % LOGPROB_TOP;
    ck[u] = LPK_NONE;
    if (s < nseg && j < kk) {
      const float2 e = *reinterpret_cast<const float2*>(part + (size_t)s * LOGPROB_PART_WORDS + 2 + 2 * j);
      const int id = __float_as_int(e.y);
      if (id != LPB_NONE) ck[u] = lp_key(e.x, id);
    }
  }
  // m = max m_s; l = sum over s of l_s 2^((m_s - m) log2e), added in segment order (lanes past nseg
  // hold 0): bit-reproducible, the same bits in every lane
  const float m = wave_max(ml.x);
  const float ts = ml_rescale(ml.x, ml.y, m);
  float l = 0.f;
#pragma unroll
  for (int s = 0; s < LOGPROB_SEGS; ++s) l += __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ts), s));
  const float lnl = logf(l);
  lpkey best = LPK_NONE;
  if (kk > 0) wave_select<LPM_N>(ck, best, lane, kk);
  // record: pair 0 = (chosen id, logprob), pairs 1..20 = (id, logprob) of entry j - 1, pair 21 = pad
  int2* rec = reinterpret_cast<int2*>(a.rec + (size_t)row * LOGPROB_REC_WORDS);
  if (lane == 0) {
    rec[0] = make_int2(tok, __float_as_int((xt - m) - lnl));
    rec[LOGPROB_TOP + 1] = make_int2(0, 0);
  }
  if (lane < LOGPROB_TOP) {
    rec[1 + lane] = best != LPK_NONE ? make_int2(lp_key_id(best), __float_as_int((lp_key_value(best) - m) - lnl))
                                     : make_int2(-1, __float_as_int(0.f));
  }
}

int logprob_segments(int S, int V) {
  if (S > SAMPLE_MAX_BLOCKS / 2) return 1;  // above 128 rows: one block per row
  int nseg = SAMPLE_MAX_BLOCKS / (S > 0 ? S : 1);
  if (nseg > LOGPROB_SEGS) nseg = LOGPROB_SEGS;
  const int cap = ((V + 3) >> 2) / 256;  // >= 1024 logits per segment
  if (nseg > cap) nseg = cap;
  return nseg < 1 ? 1 : nseg;
}

void launch_logprobs(const LogprobArgs& a, hipStream_t st) {
  if (a.S <= 0 || a.V <= 0) return;
  const int nseg = logprob_segments(a.S, a.V);
  hipLaunchKernelGGL(logprob_part_kernel, dim3(nseg, a.S), dim3(LPB_THREADS), 0, st, a,
                     tl_take("logprob_part", nseg * a.S));
  hipLaunchKernelGGL(logprob_merge_kernel, dim3(a.S), dim3(64), 0, st, a, nseg, tl_take("logprob_merge", a.S));
}

}  // namespace vgate
