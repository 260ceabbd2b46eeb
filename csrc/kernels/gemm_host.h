// Host-side pieces every GEMM launcher shares: the GemmArgs -> GemmParams copy, the CU count, the
// dynamic-LDS opt-in, the switch over the epilogue and the split-K combine launch.
#pragma once
#include <type_traits>

#include "gemm_epilogue.h"

namespace vgate {

// The one field copy. A launcher that declines the modes of a field (row gather, gamma in
// registers, RMSNorm hand-off, fused all-reduce) gets that field null / zero here because it is so
// in g; the fields no kernel of a launcher reads (AWQ operands under the bf16 kernels, counters /
// fault outside gemm_finish and the persistent prefill kernel) ride along unread. gran, qa_gran and
// vgx are the decode launchers' to set; launch_one / kx_group overwrite splitk.
inline GemmParams gemm_params(const GemmArgs& g) {
  GemmParams p{};
  p.x = g.x; p.lda = g.lda; p.M = g.M; p.row_idx = g.row_idx;
  p.wp = reinterpret_cast<const uint4*>(g.wp); p.N = g.N; p.K = g.K;
  p.norm_w = g.norm_w; p.eps = g.eps;
  p.bias = g.bias; p.res = g.res; p.ldr = g.ldr;
  p.out = g.out; p.ldo = g.ldo;
  p.splitk = 1; p.slabs = g.slabs; p.counters = g.counters;
  p.gran = nullptr; p.fault = g.fault;
  p.positions = g.positions; p.slots = g.slots; p.cos_sin = g.cos_sin;
  p.k_cache = g.k_cache; p.v_cache = g.v_cache; p.hq = g.hq; p.hkv = g.hkv; p.bs = g.bs;
  p.scales = g.scales; p.zeros = g.zeros; p.group = g.group; p.szp = g.awq_szp;
  p.hg = g.hg; p.hg_gamma = g.hg_gamma; p.ssp_out = g.ssp_out; p.ssp_in = g.ssp_in; p.ssn = g.ssn;
  p.dbg_ts = g.dbg_ts;
  p.ar = ArFused{};
  if (g.ar_world > 0) {
    for (int r = 0; r < 8; ++r) p.ar.base[r] = g.ar_fused[r];
    p.ar.err = g.ar_err; p.ar.rank = g.ar_rank; p.ar.world = g.ar_world; p.ar.spin = ar_spin();
  }
  return p;
}

// CUs of the current device, queried once per process; `fallback` when the query fails (0: the
// caller declines instead of guessing)
inline int cu_count(int fallback = 256) {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      v = 0;
    return v;
  }();
  return n > 0 ? n : fallback;
}

// Raises the kernel's dynamic LDS limit (64 KiB by default) to `bytes`, once per instantiation
template <auto Kern>
void allow_dynamic_lds(int bytes) {
  static const bool set = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  (void)set;
}

// f(std::integral_constant<int, EPI>{}) for the epilogue of a launch (EPI_BF16_AR has its own entry,
// gemm.hip): the one switch over g.epi; the caller picks NORM inside f
template <typename F>
auto with_epi(int epi, F&& f) {
  switch (epi) {
    case EPI_SILU: return f(std::integral_constant<int, EPI_SILU>{});
    case EPI_QKV: return f(std::integral_constant<int, EPI_QKV>{});
    case EPI_F32: return f(std::integral_constant<int, EPI_F32>{});
    default: return f(std::integral_constant<int, EPI_BF16>{});
  }
}

// Split-K combine + epilogue over fp32 slabs [nz][M][N] (+ row sums of squares [nz][M]): defined and
// instantiated in gemm_prefill.hip for NORM 0 / 2, NTB 1; shared with gemm_mid.hip / gemm_awq_mid.hip
template <int EPI, int NORM, int NTB>
void launch_prefill_reduce(const GemmParams& p, int nz, hipStream_t st);

}  // namespace vgate
