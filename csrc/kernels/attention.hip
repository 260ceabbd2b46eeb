// Paged attention for gfx950: decode (split-K / flash-decoding) and varlen
// causal prefill (chunked-prefill capable: queries attend to the paged cache).
//
// KV cache layout (per layer): [num_blocks][Hkv][BS=16][D=128] bf16.
//
// Both kernels use the "swapped" product S^T = K . Q^T on v_mfma_f32_16x16x32_bf16:
//   A = K tile (lane: K[tok l&15][d 8(l>>4)+j]  -> a plain 16-B row load),
//   B = Q^T   (lane: Q[col l&15][d 8(l>>4)+j]   -> a plain 16-B row load),
//   C = S^T   (lane: S[col l&15][tok 4(l>>4)+i]) -> every softmax statistic of a
//               query column lives in ONE lane group: the row max/sum need only
//               two xor-shuffles (16, 32) and the O rescale is lane-local.
// Then O^T = V^T . P^T:
//   B = P^T: built in-register from two S^T tiles with the k-order permuted to
//            {4g..4g+3, 16+4g..16+4g+3} (g = l>>4),
//   A = V^T: read from an LDS image of the V chunk with ds_read_b64_tr_b16, whose
//            4-row x 16-col transposed gather delivers exactly that k-order.
// The LDS image of V is XOR-swizzled on 8-B chunks (chunk ^= 4*(row&7)), which
// makes the transposed reads conflict-free (cdna_hip_programming.md T10).
#include "attn_decode.h"

namespace vgate {

// Combine split-K partitions: grid (S, Hq), block 128 (one thread per d).
__global__ __launch_bounds__(128) void attn_decode_reduce_kernel(AttnArgs a) {
  TLScope tl_scope(a.tl);
  const int s = blockIdx.x, hq = blockIdx.y, d = threadIdx.x;
  const int ctx = a.context_lens[s];
  if (ctx <= 0) return;
  if (a.query_start && a.query_start[s + 1] - a.query_start[s] != 1) return;
  const int nparts = (ctx + a.part_size - 1) / a.part_size;
  if (nparts <= 1) return;
  const float* pm = a.part_ml + ((size_t)s * a.Hq + hq) * a.num_parts * 2;
  const float* po = a.part_o + ((size_t)s * a.Hq + hq) * a.num_parts * D_;
  float M = -INFINITY;
  for (int p = 0; p < nparts; ++p) M = fmaxf(M, pm[2 * p]);
  float L = 0.f, acc = 0.f;
  for (int p = 0; p < nparts; ++p) {
    const float w = pm[2 * p + 1] * exp2f(pm[2 * p] - M);
    L += w;
    acc += w * po[p * D_ + d];
  }
  const int qtok = a.query_start ? a.query_start[s + 1] - 1 : s;
  a.out[(size_t)qtok * a.out_stride + (size_t)hq * D_ + d] = f2bf(L > 0.f ? acc / L : 0.f);
}

// --------------------------------------------------------------- prefill ----
// One block per (16-query tile, KV head); wave w < G owns query head h*G + w and
// its 16 query columns; every wave walks the same KV chunks, V is staged once per
// block into a double-buffered LDS image (one barrier per chunk).
__device__ __forceinline__ void prefill_body(const AttnArgs& a, int tile, int h, char* smem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nthr = blockDim.x;
  const int s = a.tile_seq[tile];
  if (s < 0) return;  // padding tile of a graph bucket (uniform over the block)
  const int q0 = a.tile_q0[tile];
  const int qs = a.query_start[s];
  const int qlen = a.query_start[s + 1] - qs;
  const int ctx = a.context_lens[s];
  const int G = a.Hq / a.Hkv;
  const bool wave_ok = wid < G;
  const int hq = h * G + (wave_ok ? wid : 0);
  const int col = lane & 15;
  const int qi = q0 + col;
  const bool qok = wave_ok && qi < qlen;
  const int qpos = ctx - qlen + qi;
  const int lim = qok ? qpos + 1 : 0;
  const int kv_end = min(ctx, ctx - qlen + min(q0 + 16, qlen));

  uint4 qf[4];
  load_q_frags(qf, a.q + (size_t)(qs + (qok ? qi : 0)) * a.q_stride + (size_t)hq * D_ + 8 * (lane >> 4), qok);
  const float cscale = a.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x4 o[8];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt) o[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16_t* vls = reinterpret_cast<bf16_t*>(smem);
  const int* bt = a.block_tables + (size_t)s * a.max_blocks;
  const size_t head_off = (size_t)h * BS_ * D_;
  const size_t blk_stride = (size_t)a.Hkv * BS_ * D_;
  const int nch = (kv_end + CHUNK - 1) / CHUNK;
  int btv = 0;  // a 64-entry window of the block table, one entry per lane (see decode_block)
  for (int c = 0; c < nch; ++c) {
    const int tb = c * CHUNK;
    if ((c & 31) == 0) btv = bt[min(2 * c + lane, a.max_blocks - 1)];
    const int b0 = __builtin_amdgcn_readlane(btv, (2 * c) & 63);
    const int b1 = (tb + BS_ < kv_end) ? __builtin_amdgcn_readlane(btv, (2 * c + 1) & 63) : b0;
    const bf16_t* vb0 = a.v_cache + (size_t)b0 * blk_stride + head_off;
    const bf16_t* vb1 = a.v_cache + (size_t)b1 * blk_stride + head_off;
    bf16_t* vl = vls + (c & 1) * (CHUNK * D_);
    for (int e = threadIdx.x; e < CHUNK * D_ / 8; e += nthr) {
      const int r = e >> 4, cc = (e & 15) * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (tb + r < kv_end) v = *reinterpret_cast<const uint4*>((r < 16 ? vb0 + r * D_ : vb1 + (r - 16) * D_) + cc);
      *reinterpret_cast<uint4*>(vl + v_lds_off(r, cc)) = v;
    }
    const bf16_t* kb0 = a.k_cache + (size_t)b0 * blk_stride + head_off;
    const bf16_t* kb1 = a.k_cache + (size_t)b1 * blk_stride + head_off;
    f32x4 s0 = qk_tile(kb0, qf, lane);
    f32x4 s1 = qk_tile(kb1, qf, lane);
    const bf16x8 pb = softmax_step(s0, s1, m, l, o, tb, min(lim, kv_end), cscale, lane);
    __syncthreads();
    pv_update(o, vl, pb, lane);
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (!qok) return;
  store_o_frags(a.out + (size_t)(qs + qi) * a.out_stride + (size_t)hq * D_, o, lane >> 4, l > 0.f ? 1.f / l : 0.f);
}

// ------------------------------------------------------- flash prefill ----
// Causal (chunked-prefill capable) attention of a block of QPB = 16 CT QG query tokens x the G
// query heads of one KV head. NW = QG G waves: wave w owns head h G + w % G for the CT 16-query
// MFMA column tiles of query group w / G; Q lives in registers. K / V stream through LDS in
// 64-token chunks, SHARED by the block's waves (GQA: one K/V byte serves G heads x QPB queries),
// moved by LDS-DMA (global_load_lds_dwordx4: no VGPRs; every wave issues P = ceil(32 / NW) of
// the chunk's 32 1-KiB pieces, padded with repeats of its own last piece so every wave's vmcnt
// bookkeeping is the same constant). FL_NST-stage ring: chunk c + FL_NST - 1 is issued at the top
// of iteration c, so a chunk's DMA has FL_NST - 1 chunks of compute to land. One barrier per chunk.
// (Deeper rings, a software-pipelined loop and an eager rescale measured no faster:
// profiles/r3_flash_prefill.log, profiles/r3_flash_split.log.)
//   S^T = K Q^T (swapped: softmax statistics lane-local, row reductions by two xor-swaps); K image
//   16-B chunks XOR-swizzled by row & 15 (conflict-free ds_read_b128 of the A operand);
//   O^T += V^T P^T with V^T read by ds_read_b64_tr_b16 from the 8-B-chunk-swizzled V image and P^T
//   built in registers (pack_p), as in the decode kernel.
// Softmax per chunk: the causal mask only on chunks that cross a query's bound (the others are
// below every query of the block), the scale folded into the exp2 argument (one fma), and the
// O / l rescale only when some column's running max moved (wave-uniform test; exact: alpha = 1
// otherwise).
// The host's 16-query tile list is reused: a block whose tile starts a QPB-aligned group leads it
// (others exit at once). The host lists the group leaders first, longest causal range first
// (ops.tile_order), so the working blocks are the grid's first ones, spread over all 8 XCDs and
// the longest start first. Chunks past the causal bound are not read (the ring's look-ahead past
// the last chunk re-reads the last one into a free stage).
extern int g_flash_prefill;
constexpr int FL_KV = 64;
constexpr int FL_STAGE = 2 * FL_KV * D_ * 2;  // K + V of one chunk (32 KiB)
constexpr int FL_NST = 2;                     // ring stages
constexpr int FL_LDS = FL_NST * FL_STAGE;     // the ring; the block-table window follows it
// K split hand-off: 16-B words per lane and part for CT column tiles (fp32 o / l: 8 each, then (m, l))
__host__ __device__ constexpr int FL_SPLIT_WORDS(int ct) { return ct * 8 + 1; }

// f32 max of values known not to be NaN: one v_max / v_max3 each (fmaxf's IEEE-mode lowering
// canonicalises every MFMA-produced input first: an extra v_max x, x per value)
__device__ __forceinline__ float fmax3_(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float fmax_(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ constexpr int vm_imm(int n) {  // s_waitcnt vmcnt(n), other counters untouched
  return (n & 0xF) | ((n >> 4) << 14) | (0x7 << 4) | (0xF << 8);
}

// dec_seqs > 0: the step's decode rows ride in the same launch — grid rows y >= num_tiles are
// (sequence, partition) decode blocks (part z == 0 of each KV head), so a prefill or mixed step has
// ONE attention launch (in a prefill-only step those blocks see no single-token sequence and exit)
template <int CT, int NW>
__global__ __launch_bounds__(64 * NW) void attn_flash_kernel(AttnArgs a, int dec_seqs) {
  constexpr int P = (32 + NW - 1) / NW;  // DMA pieces per wave per chunk
  static_assert((FL_NST - 2) * P < 64, "vmcnt immediate");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TLScope tl_scope(a.tl);
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = a.Hq / a.Hkv;
  const int QG = NW / G;
  const int QPB = 16 * CT * QG;
  // grid (Hkv x halves, tiles): the KV heads (and a split range's two halves) of one tile are
  // adjacent in dispatch order, so the tile list's longest-first order holds across every head
  const int zs = gridDim.x / a.Hkv;
  const int h = blockIdx.x / zs;
  const int tile = blockIdx.y;
  if (tile >= a.num_tiles) {  // block-uniform: a decode block
    const int r = tile - a.num_tiles;
    if (blockIdx.x % zs == 0 && dec_seqs > 0) decode_block(a, r % dec_seqs, h, r / dec_seqs, smem);
    return;
  }
  const int s = a.tile_seq[tile];
  if (s < 0) return;
  const int q0 = a.tile_q0[tile];
  if (q0 % QPB) return;  // block-uniform: not a group leader
  const int qs = a.query_start[s];
  const int qlen = a.query_start[s + 1] - qs;
  // a single-query sequence is a decode row, computed by this launch's decode blocks: a tile of it
  // (a tile list that names every sequence) must not write the same output row concurrently
  if (qlen == 1 && dec_seqs > 0) return;  // block-uniform
  const int ctx = a.context_lens[s];
  const int hq = h * G + wid % G;
  const int qw0 = q0 + 16 * CT * (wid / G);  // this wave's first query
  const int qhi = min(q0 + QPB, qlen);       // the block's queries: [q0, qhi)
  const int kv_end = ctx - qlen + qhi;       // the block's causal bound (exclusive)
  const int nch = (kv_end + FL_KV - 1) / FL_KV;
  const int nfull = max(0, ctx - qlen + q0 + 1) / FL_KV;  // chunks below every query's bound
  // K split (zs parts per KV head, launch_attention): a range of nch chunks runs as nsp =
  // min(zs, nch / 2) parts of whole chunks (>= 2 each), part z on [nch z / nsp, nch (z+1) / nsp),
  // met in the epilogue; the causal triangle's long tail then costs 1 / nsp of a range per block.
  // Parts past nsp exit at once. Block-uniform, before any barrier.
  const int z = blockIdx.x % zs;
  const int nsp = min(zs, nch / 2);
  const bool split = nsp > 1;
  if (z >= max(nsp, 1)) return;
  const int c0 = split ? nch * z / nsp : 0;
  const int c1 = split ? nch * (z + 1) / nsp : nch;
  const int col = lane & 15, g4 = lane >> 4;
  // Q fragments (B operand of S^T = K Q^T): CT column tiles x 4 k-slices
  uint4 qf[CT][4];
  int lim[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int qi = qw0 + 16 * ct + col;
    const bool ok = qi < qhi;
    lim[ct] = ok ? ctx - qlen + qi + 1 : 0;
    load_q_frags(qf[ct], a.q + (size_t)(qs + (ok ? qi : 0)) * a.q_stride + (size_t)hq * D_ + 8 * g4, ok);
  }
  const size_t blk_stride = (size_t)a.Hkv * BS_ * D_;
  const size_t head_off = (size_t)h * BS_ * D_;
  // the sequence's block-table entries of the causal range, staged in LDS once: a DMA's source page
  // is then an LDS broadcast read, not a global load whose wait would serialise behind the DMAs
  // already in flight (vmcnt counts both)
  int* s_bt = reinterpret_cast<int*>(smem + FL_LDS);
  const int npg = (kv_end + BS_ - 1) / BS_;
  {
    const int* bt = a.block_tables + (size_t)s * a.max_blocks;
    for (int i = threadIdx.x; i < npg; i += blockDim.x) s_bt[i] = bt[i];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // Q fragments and the block table
  __builtin_amdgcn_s_barrier();
  // chunk c's 32 DMA pieces (16 K, 16 V) over the block's waves, into stage c % NST; past the last
  // chunk the last one is re-read (the ring keeps NST - 1 chunks in flight, a constant vmcnt).
  // Piece i of a chunk: K rows 4 i .. 4 i + 3 (i < 16; lane -> physical 16-B chunk l & 15 holds
  // logical chunk ^ (row & 15)) or V half (i - 16) / 8, rows 4 ((i - 16) % 8) .. + 3 of that half
  // (v_lds_off's 8-B chunk swizzle). Everything but the 4 pages of the chunk is chunk-invariant:
  // the lane's element offset inside its page and the piece's page slot / LDS offset are set once.
  uint32_t loff[P];  // lane's element offset inside the page
  int pslot[P], pisv[P], pdst[P];  // wave-uniform: page slot 0..3, V?, LDS byte offset in the stage
#pragma unroll
  for (int k = 0; k < P; ++k) {
    int i = wid + k * NW;
    if (i >= 32) i = wid + (k - 1) * NW;  // pad: this wave's previous piece again (same bytes, same place)
    const int isv = i >> 4, pi = i & 15;
    int r, d0;
    if (!isv) {
      r = 4 * pi + g4;
      d0 = 8 * (col ^ (r & 15));
    } else {
      const int rh = 4 * (pi & 7) + g4;
      r = 32 * (pi >> 3) + rh;
      d0 = (8 * col) ^ (16 * (rh & 7));
    }
    loff[k] = (uint32_t)((r & 15) * D_ + d0);
    pslot[k] = isv ? 2 * (pi >> 3) + ((pi & 7) >> 2) : pi >> 2;  // rows of a piece share one page
    pisv[k] = isv;
    pdst[k] = (isv ? FL_KV * D_ * 2 : 0) + pi * 1024;
  }
  auto issue = [&](int c) {
    const uint32_t stage = lds_addr_of(smem) + (uint32_t)((c % FL_NST) * FL_STAGE);
    const int cc = min(c, c1 - 1);
    int pg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pg[j] = __builtin_amdgcn_readfirstlane(s_bt[min(4 * cc + j, npg - 1)]);  // past the bound: the last page
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int page = pslot[k] == 0 ? pg[0] : pslot[k] == 1 ? pg[1] : pslot[k] == 2 ? pg[2] : pg[3];
      const bf16_t* base = (pisv[k] ? a.v_cache : a.k_cache) + (size_t)page * blk_stride + head_off;
      glds16(base + loff[k], stage + (uint32_t)pdst[k]);
    }
  };
  const float cscale = a.scale * LOG2E;
  float m[CT], l[CT];  // running max (scaled, log2 domain) and sum per column
  f32x4 o[CT][8];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    m[ct] = -INFINITY;
    l[ct] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) o[ct][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int row4 = 4 * g4 + ((lane >> 2) & 3);  // vt_frag's row (pv_update)
  // S^T tiles of chunk c: 4 token tiles x CT column tiles (K from stage c % NST)
  auto qk = [&](int c, f32x4 (&st)[4][CT]) {
    const char* kb = smem + (c % FL_NST) * FL_STAGE;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) st[tt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* krow = kb + (16 * tt + col) * 256;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const uint4 kf = *reinterpret_cast<const uint4*>(krow + (((4 * kk + g4) ^ col) << 4));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) st[tt][ct] = mfma16(as_bf16x8(kf), as_bf16x8(qf[ct][kk]), st[tt][ct]);
      }
    }
  };
  // online softmax of chunk c per column tile over its 64 tokens (lane: column col, tokens
  // 16 tt + 4 g4 + i) -> P^T fragments
  auto softmax = [&](int c, f32x4 (&st)[4][CT], bf16x8 (&pb)[CT][2]) {
    const bool masked = c >= nfull;  // block-uniform
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (masked) {
        // token t = c 64 + 16 tt + 4 g4 + i is masked when t >= lim: i.e. 16 tt + i >= lim - c 64 - 4 g4
        const int rel = lim[ct] - c * FL_KV - 4 * g4;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (16 * tt + i >= rel) st[tt][ct][i] = -INFINITY;
      }
      // max without NaN canonicalisation (the scores are finite or -inf): v_max3 chains
      float cmax = -INFINITY;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
        cmax = fmax3_(cmax, fmax3_(st[tt][ct][0], st[tt][ct][1], st[tt][ct][2]), st[tt][ct][3]);
      cmax = fmax_(cmax, xor16(cmax));
      cmax = fmax_(cmax, xor32(cmax));
      const float mn = fmaxf(m[ct], cmax * cscale);
      if (__any(mn > m[ct])) {  // lazy rescale (wave-uniform): only when a running max moved
        const float alpha = __builtin_amdgcn_exp2f(m[ct] - (mn == -INFINITY ? 0.f : mn));
        l[ct] *= alpha;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) o[ct][mt] *= alpha;
        m[ct] = mn;
      }
      const float mref = m[ct] == -INFINITY ? 0.f : m[ct];  // fully masked column: exp2(-inf) = 0, no NaN
      float ps = 0.f;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          st[tt][ct][i] = __builtin_amdgcn_exp2f(fmaf(st[tt][ct][i], cscale, -mref));
          ps += st[tt][ct][i];
        }
      l[ct] += ps;
      pb[ct][0] = pack_p(st[0][ct], st[1][ct]);
      pb[ct][1] = pack_p(st[2][ct], st[3][ct]);
    }
  };
  // O^T += V^T P^T of chunk c: each V^T fragment (ds_read_b64_tr_b16) feeds every column tile
  auto pv = [&](int c, const bf16x8 (&pb)[CT][2]) {
    const bf16_t* vb = reinterpret_cast<const bf16_t*>(smem + (c % FL_NST) * FL_STAGE + FL_KV * D_ * 2);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const bf16_t* vh = vb + half * (32 * D_);
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) {
        const bf16x8 av = vt_frag(vh, row4, 16 * mt + 4 * (lane & 3));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct][mt] = mfma16(av, pb[ct][half], o[ct][mt]);
      }
    }
  };
  if (c1 > c0) {
#pragma unroll
    for (int c = 0; c < FL_NST - 1; ++c) issue(c0 + c);
  }
  __builtin_amdgcn_s_waitcnt(vm_imm((FL_NST - 2) * P));  // chunk c0 landed (this wave's pieces)
  __builtin_amdgcn_s_barrier();                          // everyone's
  for (int c = c0; c < c1; ++c) {
    issue(c + FL_NST - 1);  // into the stage every wave finished reading last iteration
    f32x4 st[4][CT];
    bf16x8 pb[CT][2];
    qk(c, st);
    softmax(c, st, pb);
    pv(c, pb);
    __builtin_amdgcn_s_waitcnt(vm_imm((FL_NST - 2) * P));  // this wave's pieces of chunk c + 1 landed
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // everyone's; stage c % NST free
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the look-ahead DMAs drained before the block exits
  if (split) {
    // The parts meet per wave. Each hands over its partial normalised by its own sum (o / l) and
    // (m, l), all fp32 (rounded to bf16, a partial carried its rounding at ITS magnitude into the
    // merge: two halves that cancel left up to 2^-9 of a half in a result near zero), and takes the
    // wave's ticket first: the nsp - 1 early arrivers publish (16-B sc1 stores, drain, +1 on the ready
    // word) and exit; the last waits for ready = nsp - 1 (the others never wait, so they always get
    // there), re-arms both words and merges every part's partial in fixed part order, its own as the
    // very values it would have published: the result does not depend on arrival order.
    // Slot: the leader's rank over the step (every earlier sequence holds ceil(qlen / QPB)
    // leaders), KV head, wave; the host sized fl_ws for (tiles 16 / QPB + S + 1) Hkv NW <= 32768
    // slots of zs parts.
    int before = 0;
    for (int i = lane; i < s; i += 64) {
      const int ql = a.query_start[i + 1] - a.query_start[i];
      before += (ql + QPB - 1) / QPB;
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) before += __shfl_xor(before, sh);
    const uint32_t wslot = (uint32_t)(((before + q0 / QPB) * a.Hkv + h) * NW + wid);
    uint32_t* ticket = a.fl_tickets + wslot;
    uint32_t* ready = a.fl_tickets + 32768 + wslot;
    float ll[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {  // this part's o / l, in place
      ll[ct] = l[ct];
      ll[ct] += xor16(ll[ct]);
      ll[ct] += xor32(ll[ct]);
      const float inv = ll[ct] > 0.f ? 1.f / ll[ct] : 0.f;
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) o[ct][mt] *= inv;
    }
    constexpr uint32_t PW = FL_SPLIT_WORDS(CT);  // 16-B words per lane and part: the fp32 partial, then (m, l) pairs
    const uint32_t lane_off = lane * 16u;
    auto part_off = [&](int p) { return (wslot * (uint32_t)zs + (uint32_t)p) * PW * 1024u + lane_off; };
    uint32_t old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0);
    if (old + 1 < (uint32_t)nsp) {
      const uint32_t off = part_off(z);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) st_sc1_x4(a.fl_ws, off + (uint32_t)(ct * 8 + mt) * 1024u, o[ct][mt]);
      st_sc1_x4(a.fl_ws, off + CT * 8 * 1024u, f32x4{m[0], ll[0], m[CT - 1], ll[CT - 1]});
      drain_stores();
      if (lane == 0) __hip_atomic_fetch_add(ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    if (lane == 0) {
      uint32_t spins = 0;
      bool late = false;
      while (__hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 < (uint32_t)nsp) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1u << 22)) { late = true; break; }  // bounded: never hang the GPU
      }
      if (late) {
        // the result is wrong and a late part may still add to `ready`: leave the words as they are and
        // raise the sticky fault word, which the step's last node hands to the host (engine fails)
        if (a.fault != nullptr) atomicOr(a.fault, 2u);
      } else {
        __hip_atomic_store(ready, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("" ::: "memory");  // the partials' loads stay behind the flag
    // every part's (m, l) -> weights, then the partials in part order
    f32x4 ml[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      ml[p] = (p < nsp && p != z) ? ld_sc1_x4(a.fl_ws, part_off(p) + CT * 8 * 1024u)
                                  : f32x4{m[0], ll[0], m[CT - 1], ll[CT - 1]};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float mm = -INFINITY;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < nsp) mm = fmaxf(mm, ml[p][2 * ct]);
      const float mref = mm == -INFINITY ? 0.f : mm;
      float wt[4], lt = 0.f;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        wt[p] = p < nsp ? __builtin_amdgcn_exp2f(ml[p][2 * ct] - mref) * ml[p][2 * ct + 1] : 0.f;
        lt += wt[p];
      }
      const float inv = lt > 0.f ? 1.f / lt : 0.f;
      f32x4 acc[8];
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p >= nsp) continue;
        f32x4 v[8];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
          v[mt] = p == z ? o[ct][mt] : ld_sc1_x4(a.fl_ws, part_off(p) + (uint32_t)(ct * 8 + mt) * 1024u);
        const float wp = wt[p] * inv;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) acc[mt] += v[mt] * wp;
      }
      const int qi = qw0 + 16 * ct + col;
      if (qi < qhi) store_o_frags(a.out + (size_t)(qs + qi) * a.out_stride + (size_t)hq * D_, acc, g4);
    }
    return;
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float ll = l[ct];
    ll += xor16(ll);
    ll += xor32(ll);
    const int qi = qw0 + 16 * ct + col;
    if (qi < qhi)
      store_o_frags(a.out + (size_t)(qs + qi) * a.out_stride + (size_t)hq * D_, o[ct], g4, ll > 0.f ? 1.f / ll : 0.f);
  }
}

// flash configuration for a head group of G (ct = 0: not supported): waves NW = 8 when G | 8
// (G query groups of 8 / G), 6 for G = 3, 6; two 16-query column tiles per wave for G <= 4
// (Llama: 64-query blocks), one above (16-query blocks keep >= one block per CU at 2k tokens for
// the 1-2 KV-head layouts; two there were slower at every length, profiles/r3_flash_split.log).
// The head-group rule is restated by ops.flash_lead (vgate/ops/__init__.py, which must work without
// this module) and by tests/test_attn_probe_gpu.py _has_flash: change the three together.
struct FlashCfg { int ct, nw; };
static FlashCfg flash_cfg(const AttnArgs& a) {
  if (a.D != D_ || a.BS != BS_ || a.Hkv <= 0 || a.Hq % a.Hkv) return {0, 0};
  const int G = a.Hq / a.Hkv;
  const int nw = 8 % G == 0 ? 8 : (6 % G == 0 ? 6 : 0);
  if (nw == 0) return {0, 0};
  const int ct = G <= 4 ? 2 : 1;
  return {ct, nw};
}

static bool flash_enabled() {
  static const int v = [] { const char* e = getenv("VGATE_FLASH_PREFILL"); return e ? atoi(e) : 1; }();
  return g_flash_prefill >= 0 ? g_flash_prefill != 0 : v != 0;
}

// ------------------------------------------------------------- unified launch ----
// grid.x = [decode blocks: one per (sequence, partition), partition-major: bx = p*S + s]
//          ++ [prefill tiles], grid.y = KV heads. One launch serves a decode-only,
// prefill-only or mixed (chunked-prefill) step; waves / blocks without work exit.
// MAXT: 512 threads (G <= 8 query heads per KV head) leaves 256 VGPRs per wave for the
// prefetched K + in-flight V + O accumulators; 1024 only for G > 8.
template <int MAXT>
__global__ __launch_bounds__(MAXT) void attn_kernel(AttnArgs a, int dec_seqs, int dec_blocks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TLScope tl_scope(a.tl);
  const int bx = blockIdx.x;
  if (bx < dec_blocks) {
    decode_block(a, bx % dec_seqs, blockIdx.y, bx / dec_seqs, smem);  // block = (sequence, partition)
  } else {
    // (a tile of a single-query sequence: that row is a decode block's, see attn_flash_kernel)
    const int s = a.tile_seq[bx - dec_blocks];
    if (dec_seqs > 0 && s >= 0 && a.query_start[s + 1] - a.query_start[s] == 1) return;
    prefill_body(a, bx - dec_blocks, blockIdx.y, smem);
  }
}

static int attn_waves(const AttnArgs& a) {
  const int G = a.Hq / a.Hkv;
  return G > 4 ? G : 4;
}

int g_flash_prefill = -1;  // -1: VGATE_FLASH_PREFILL (default on); 0 / 1: set_flash_prefill (tests)
void set_flash_prefill(int on) { g_flash_prefill = on; }

// K split of the long causal ranges (zs parts per KV head, adjacent in grid.x) when the
// workspace holds every wave's partials: 2 parts while the step's working blocks fill less
// than two waves of the chip's block slots (CT = 2 blocks hold a CU alone, CT = 1 two), 4
// while 4 parts per block still fit in one wave (profiles/r3_flash_split.log: 4 parts won
// only there: Llama-3-70B TP=8 2048 39.8 -> 31.9 us, lost at Qwen 2048 46 -> 50, Llama-8B
// 1024 35 -> 45); none once the blocks alone fill two waves (they balance the triangle)
static int flash_split_parts(const AttnArgs& a, FlashCfg fc, int tiles) {
  if (a.fl_ws == nullptr || a.fl_tickets == nullptr) return 1;
  const int qpb = 16 * fc.ct * (fc.nw / (a.Hq / a.Hkv));
  const size_t leaders = (size_t)tiles * 16 / qpb + (size_t)a.S + 1;
  const size_t slots = leaders * a.Hkv * fc.nw;
  const size_t blocks = (size_t)tiles * 16 / qpb * a.Hkv;
  const size_t cap = (size_t)cu_count(1) * (fc.ct == 2 ? 1 : 2);
  int zs = 1;
  if (blocks < 2 * cap) zs = 2;
  if (blocks * 4 <= cap) zs = 4;
  if (slots > 32768 || slots * zs * FL_SPLIT_WORDS(fc.ct) * 1024 > a.fl_ws_bytes) zs = 1;
  return zs;
}

void launch_attention(const AttnArgs& a, int dec_seqs, hipStream_t st) {
  const int tiles = a.num_tiles > 0 ? a.num_tiles : 0;
  const int dec_blocks = dec_seqs > 0 ? dec_seqs * a.num_parts : 0;
  if (tiles + dec_blocks <= 0) return;
  AttnArgs b = a;
  b.num_tiles = tiles;
  // prefill tiles on the flash kernel when it takes the head layout (a decode-only graph bucket
  // carries no tile list, StepMeta.view); either way the decode rows ride in the same launch
  const FlashCfg fc = tiles > 0 && flash_enabled() ? flash_cfg(a) : FlashCfg{0, 0};
  if (fc.ct > 0) {
    const int zs = flash_split_parts(a, fc, tiles);
    const size_t lds = std::max((size_t)FL_LDS + (size_t)a.max_blocks * 4, (size_t)attn_lds_bytes(fc.nw));
    b.tl = tl_take("attn_flash", (tiles + dec_blocks) * a.Hkv * zs);
    const auto kern = fc.nw == 8 ? (fc.ct == 2 ? attn_flash_kernel<2, 8> : attn_flash_kernel<1, 8>)
                                 : (fc.ct == 2 ? attn_flash_kernel<2, 6> : attn_flash_kernel<1, 6>);
    hipLaunchKernelGGL(kern, dim3(a.Hkv * zs, tiles + dec_blocks, 1), dim3(64 * fc.nw), lds, st, b, dec_seqs);
  } else {
    const int nw = attn_waves(a);
    b.tl = tl_take("attention", (tiles + dec_blocks) * a.Hkv);
    const auto kern = nw <= 8 ? attn_kernel<512> : attn_kernel<1024>;
    hipLaunchKernelGGL(kern, dim3(dec_blocks + tiles, a.Hkv, 1), dim3(64 * nw), attn_lds_bytes(nw), st, b, dec_seqs,
                       dec_blocks);
  }
  if (dec_seqs > 0 && a.num_parts > 1 && a.tickets == nullptr) {  // the partitions' separate reduce launch
    b.tl = tl_take("attn_reduce", dec_seqs * a.Hq);
    hipLaunchKernelGGL(attn_decode_reduce_kernel, dim3(dec_seqs, a.Hq), dim3(128), 0, st, b);
  }
}

}  // namespace vgate
