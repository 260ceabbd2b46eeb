"""Weight packing for the GEMM kernels and the :class:`Linear` that holds a layer in kernel-ready form."""
from __future__ import annotations

import torch

from . import reference as ref
from ._native import PATH_AUTO


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> fragment-major [N/16, K/32, 4, 16, 8] (see csrc/kernels/gemm.hip)."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    return w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def unpack_weight(wp: torch.Tensor, N: int, K: int) -> torch.Tensor:
    return wp.reshape(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K)


def interleave_gate_up(w_gate: torch.Tensor, w_up: torch.Tensor) -> torch.Tensor:
    """Rows ordered [G0 U0 G1 U1 ...] in 16-row tiles for the fused SiLU*mul epilogue."""
    I, K = w_gate.shape
    assert I % 16 == 0
    return torch.stack([w_gate.reshape(I // 16, 16, K), w_up.reshape(I // 16, 16, K)], 1).reshape(2 * I, K)


def unpack_awq(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_awq`: int32 [N/16, K/128, 64, 4] -> int4 values [N, K] (int32)."""
    w = packed.to(torch.int64) & 0xFFFFFFFF
    w = w.reshape(N // 16, K // 128, 4, 16, 4)  # nt, kq, g, r, u
    j = torch.arange(8, dtype=torch.int64, device=packed.device)
    shifts = (j & 1) * 16 + (j >> 1) * 4
    q = (w[..., None] >> shifts) & 0xF  # nt, kq, g, r, u, j
    return q.permute(0, 3, 1, 4, 2, 5).reshape(N, K).to(torch.int32)


def pack_awq(qint: torch.Tensor) -> torch.Tensor:
    """int4 values [N, K] (0..15) -> int32 [N/16, K/128, 64, 4]; word u of lane l holds the 8
    values W[16nt + (l&15)][128kq + 32u + 8(l>>4) + j], j = 0..7, with the EVEN j in the low
    half-word and the odd j in the high one: value j at bit (16 if j odd) + 4 (j >> 1).
    Then (word >> 4d) & 0x000F000F | 0x43004300 is the bf16 pair (128 + v_2d, 128 + v_2d+1):
    two VALU ops per MFMA operand dword (gemm.hip, AWQ decode kernel)."""
    N, K = qint.shape
    assert N % 16 == 0 and K % 128 == 0
    q = qint.to(torch.int64).reshape(N // 16, 16, K // 128, 4, 4, 8)  # nt, r, kq, u, g, j
    q = q.permute(0, 2, 4, 1, 3, 5)  # nt, kq, g, r, u, j  -> lane = g*16 + r
    j = torch.arange(8, dtype=torch.int64, device=qint.device)
    shifts = (j & 1) * 16 + (j >> 1) * 4
    words = (q << shifts).sum(-1)  # [nt, kq, g, r, u]
    words = words.reshape(N // 16, K // 128, 64, 4)
    words = torch.where(words >= 2**31, words - 2**32, words)
    return words.to(torch.int32).contiguous()


def pack_awq_sz(scales: torch.Tensor, sz: torch.Tensor) -> torch.Tensor:
    """Group scales in the AWQ decode kernels' fragment order (csrc/kernels/gemm_kx.h /
    gemm_kx_q4.hip, gemm_awq_mid.hip):
    [N/16][K/128][4 lane groups][s(4 cols), s*z(4 cols)] bf16, so the lanes of a 16-lane group load
    their 4 columns' scale AND zero term with ONE 16-B load per (tile, k-quad). Group 128 only."""
    G, N = scales.shape
    s4 = scales.t().reshape(N // 16, 4, 4, G).permute(0, 3, 1, 2)  # [nt][g][lane group][4]
    z4 = sz.t().reshape(N // 16, 4, 4, G).permute(0, 3, 1, 2)
    return torch.cat([s4, z4], dim=-1).to(torch.bfloat16).contiguous()  # [nt][g][4][8]


def pack_fp8(codes: torch.Tensor) -> torch.Tensor:
    """e4m3fn codes uint8 [N, K] -> uint8 [N/16, K/64, 64, 16]: byte 8u + j of lane l is the code of
    W[16nt + (l&15)][64kp + 32u + 8(l>>4) + j], u = 0, 1, j = 0..7, so one 16-B lane load is the A
    operand of two MFMA k-steps (csrc/kernels/gemm_fp8.hip)."""
    N, K = codes.shape
    assert codes.dtype == torch.uint8 and N % 16 == 0 and K % 64 == 0, (codes.dtype, N, K)
    c = codes.reshape(N // 16, 16, K // 64, 2, 4, 8)  # nt, r, kp, u, g, j
    return c.permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 64, 16).contiguous()  # lane = g * 16 + r


def unpack_fp8(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_fp8`: uint8 [N/16, K/64, 64, 16] -> codes uint8 [N, K]."""
    c = packed.reshape(N // 16, K // 64, 4, 16, 2, 8)  # nt, kp, g, r, u, j
    return c.permute(0, 3, 1, 4, 2, 5).reshape(N, K)


def fp8_dequant_ref(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """bf16(fp32(code) * scale): codes uint8 [N, K] (e4m3fn), scales fp32 [G, N], G = 1 or K / 128."""
    N, K = codes.shape
    G = scales.shape[0]
    g = torch.arange(K, device=codes.device) // (K // G)
    return (codes.view(torch.float8_e4m3fn).float() * scales.float()[g].t()).to(torch.bfloat16)


E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitude of code & 7; bit 3 is the sign


def pack_mxfp4(codes: torch.Tensor) -> torch.Tensor:
    """e2m1 codes uint8 [N, K] (one nibble value per byte) -> uint8 [N/16, K/128, 64, 16]: dword u of lane
    l holds the codes of W[16nt + (l&15)][128kq + 32u + 8(l>>4) + j], j = 0..7, code j in nibble j (low
    nibble of byte 0 first), so one 16-B lane load is the A operand of four MFMA k-steps
    (csrc/kernels/gemm_mxfp4.hip)."""
    N, K = codes.shape
    assert codes.dtype == torch.uint8 and N % 16 == 0 and K % 128 == 0, (codes.dtype, N, K)
    c = codes.reshape(N // 16, 16, K // 128, 4, 4, 4, 2)  # nt, r, kq, u, g, byte, nibble
    b = (c[..., 0] & 0xF) | (c[..., 1] << 4)
    return b.permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 128, 64, 16).contiguous()  # lane = g * 16 + r


def unpack_mxfp4(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_mxfp4`: uint8 [N/16, K/128, 64, 16] -> codes uint8 [N, K]."""
    b = packed.reshape(N // 16, K // 128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5)  # nt, r, kq, u, g, byte
    return torch.stack([b & 0xF, b >> 4], dim=-1).reshape(N, K)


def pack_mxfp4_scales(scales: torch.Tensor) -> torch.Tensor:
    """e8m0 bytes uint8 [N, K/32] -> uint8 [N/16, K/128, 16, 4]: byte u of row r is the scale of the 32-block
    (row 16nt + r, k-step 4kq + u), one 4-B load per lane and 128-k unit."""
    N, KB = scales.shape
    assert scales.dtype == torch.uint8 and N % 16 == 0 and KB % 4 == 0, (scales.dtype, N, KB)
    return scales.reshape(N // 16, 16, KB // 4, 4).permute(0, 2, 1, 3).contiguous()


def unpack_mxfp4_scales(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of :func:`pack_mxfp4_scales`: uint8 [N/16, K/128, 16, 4] -> uint8 [N, K/32]."""
    return packed.reshape(N // 16, K // 128, 16, 4).permute(0, 2, 1, 3).reshape(N, K // 32)


def mxfp4_dequant_ref(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """bf16(value(code) * 2^(e - 127)): codes uint8 [N, K] (e2m1 nibble values), scales uint8 [N, K/32]
    (e8m0). Exact for 2 <= e <= 252."""
    tab = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float64, device=codes.device)
    s = torch.exp2(scales.double() - 127.0).repeat_interleave(32, dim=1)
    return (tab[codes.long()] * s).to(torch.bfloat16)


def mxfp4_check_scales(codes: torch.Tensor, scales: torch.Tensor, name: str) -> torch.Tensor:
    """The admitted scale bytes of codes [N, K] / scales [N, K/32]: 255 (NaN) raises; a block whose 32
    codes are all +-0 may carry any other byte, rewritten to 127; otherwise 2 <= e <= 252 (the range in
    which value * 2^(e-127) is exact in bf16) or it raises. Returns the scales to keep."""
    if bool((scales == 255).any()):
        raise ValueError(f"{name}: e8m0 scale byte 255 (NaN)")
    zero = ((codes & 7) == 0).reshape(codes.shape[0], -1, 32).all(dim=2)
    bad = ~zero & ((scales < 2) | (scales > 252))
    if bool(bad.any()):
        n, kb = (int(v) for v in bad.nonzero()[0])
        raise ValueError(f"{name}: e8m0 scale byte {int(scales[n, kb])} of block (row {n}, k-block {kb}) is outside "
                         f"2..252 (code * 2^(e-127) would not be exact in bf16)")
    return torch.where(zero, torch.full_like(scales, 127), scales)


def mxfp4_quantize(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(codes uint8 [N, K], scales uint8 [N, K/32]) of a matrix [N, K], K % 32 == 0 (Linear.quantize_mxfp4)."""
    N, K = w.shape
    x = w.double().reshape(N, K // 32, 32)
    amax = x.abs().amax(dim=2)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, 0.5 <= m < 1: floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, ex.long() - 1 - 2 + 127, torch.full_like(ex.long(), 127)).clamp(2, 252)
    a = (x.abs() * torch.exp2(127.0 - e.double())[..., None])
    q = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2)).clamp(max=6.0)
    idx = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4)).long()
    codes = (idx | (torch.signbit(x).long() << 3)).to(torch.uint8).reshape(N, K)
    return codes, e.to(torch.uint8)


def row_permutation(N: int, layout: str) -> torch.Tensor | None:
    """Row order of the packed weight for a fused epilogue (None = identity).

    silu: tile t = gate rows 8t..8t+7 then up rows 8t..8t+7 (rows [gate; up] in the dense
          matrix), so one 16-row tile holds 8 SiLU pairs on lanes l, l^32 and a decode block
          can own a single tile (gemm_epilogue.h);
    qkv : per 128-wide head, tile t (t = 0..7) = rows 8t..8t+7 then their NeoX rotation
          partners 64+8t..64+8t+7, so one 16-row tile holds both halves of 8 rotation pairs
          (the GEMM epilogue exchanges them across lanes l, l^32; csrc/kernels/gemm.hip qkv_col).
    """
    if layout == "silu":
        I = N // 2
        assert I % 8 == 0
        t = torch.arange(2 * I).reshape(2, I // 8, 8).transpose(0, 1)
        return t.reshape(-1)
    if layout == "qkv":
        assert N % 128 == 0
        heads = N // 128
        tile = torch.arange(128).reshape(2, 8, 8).permute(1, 0, 2).reshape(8, 16)
        t = torch.arange(heads)[:, None, None] * 128 + tile[None]
        return t.reshape(-1)
    return None


class Linear:
    """A linear layer's weights in kernel-ready form.

    layout: "plain" | "silu" (rows [gate; up] -> out = silu(gate) * up)
            | "qkv" (rows [q; k; v], heads of 128: fused bias + RoPE + KV-cache write).
    Dense bf16 weights, AWQ int4 (``awq={"qint", "scales", "zeros", "group"}``) or FP8 W8A16
    (``fp8={"codes", "scales", "layout"}``: e4m3fn codes uint8 [N, K], fp32 scales [1, N] per channel or
    [K/128, N] per 128-k block, original row order; the weight is code * scale) or MXFP4 W4A16
    (``mxfp4={"codes", "scales", "layout"}``: e2m1 codes uint8 [N, K], one nibble value per byte, e8m0 scales
    uint8 [N, K/32], original row order; the weight is value(code) * 2^(scale - 127)).
    On GPU only the fragment-packed copy is kept; on CPU the dense matrix (reference path).
    """

    def __init__(self, w: torch.Tensor | None, bias: torch.Tensor | None = None, kind: str = "plain",
                 awq: dict | None = None, layout: str | None = None, fp8: dict | None = None,
                 mxfp4: dict | None = None):
        if kind in ("silu", "qkv"):
            layout, kind = kind, "dense"
        quant = awq if awq is not None else fp8 if fp8 is not None else mxfp4
        self.layout = layout or (quant.get("layout", "plain") if quant else "plain")
        if awq is not None and awq.get("silu"):
            self.layout = "silu"
        self.kind = "awq" if awq is not None else "fp8" if fp8 is not None else "mxfp4" if mxfp4 is not None else "dense"
        self.bias = bias
        self.norm_gamma = None  # RMSNorm weight folded into the packed copy (see fold_norm)
        # a plain-layout Linear whose input is RMSNormed in its launch (a QK-norm model's QKV projection;
        # "qkv" / "silu" layouts always are): the tuner times its candidates with the row scale
        self.norm_in = False
        # decode-GEMM decomposition for M <= 16 steps (0 = the launcher's heuristic): set by the
        # model from the measured per-shape table (vgate/models/decode_plans.py)
        self.dec_waves = 0
        self.dec_splitk = 0
        self.dec_sk = None  # stream-K decode kernel: None = STREAMK_DECODE, or (waves, blocks/CU, group)
        self.dec_ntb = 0
        self.dec_path = PATH_AUTO  # PATH_KX: the register-stationary decode kernel (csrc/kernels/gemm_kx.h)
        # prefill (M >= 128) tile / K-slice choice per M bucket, measured at engine start-up
        # (tune_prefill); empty = the launcher's heuristic
        self.prefill_plan: dict[int, tuple[int, int]] = {}
        self.w = self.wp = None  # the dense matrix on the CPU, the packed copy on a GPU
        self.szp = None  # AWQ group 128 on a GPU: the packed (scale, scale * zero) operand (pack_awq_sz)
        self.fscales = None  # FP8 on a GPU: fp32 scales [G, N] in the packed row order
        self.mscales = None  # MXFP4 on a GPU: packed e8m0 bytes (pack_mxfp4_scales) in the packed row order
        if self.kind == "mxfp4":
            codes, scales = mxfp4["codes"], mxfp4["scales"]
            if hasattr(torch, "float8_e8m0fnu") and scales.dtype == torch.float8_e8m0fnu:
                scales = scales.view(torch.uint8)
            if codes.dim() != 2 or codes.dtype != torch.uint8 or codes.shape[0] % 16 or codes.shape[1] % 128:
                raise ValueError(f"mxfp4 Linear: e2m1 codes uint8 [N % 16 == 0, K % 128 == 0], got {codes.dtype} "
                                 f"{tuple(codes.shape)}")
            self.N, self.K = codes.shape
            if scales.dtype != torch.uint8 or tuple(scales.shape) != (self.N, self.K // 32):
                raise ValueError(f"mxfp4 Linear: e8m0 scales uint8 [N, K/32] = [{self.N}, {self.K // 32}], got "
                                 f"{scales.dtype} {tuple(scales.shape)}")
            dev = scales.device
            codes = codes.to(dev)
            if bool((codes > 15).any()):
                raise ValueError("mxfp4 Linear: codes are one e2m1 nibble value (0..15) per byte")
            scales = mxfp4_check_scales(codes, scales, "mxfp4 Linear")
            if dev.type == "cuda":
                perm = row_permutation(self.N, self.layout)
                if perm is not None:
                    pd = perm.to(dev)
                    codes, scales = codes[pd], scales[pd]
                self.wp = pack_mxfp4(codes.contiguous())
                self.mscales = pack_mxfp4_scales(scales.contiguous())
            else:
                self.w = mxfp4_dequant_ref(codes, scales)
            return
        if self.kind == "fp8":
            codes, scales = fp8["codes"], fp8["scales"]
            if codes.dtype == torch.float8_e4m3fn:
                codes = codes.view(torch.uint8)
            self.N, self.K = codes.shape
            if codes.dtype != torch.uint8 or self.N % 16 or self.K % 128:
                raise ValueError(f"fp8 Linear: e4m3fn codes [N % 16 == 0, K % 128 == 0], got {codes.dtype} "
                                 f"{tuple(codes.shape)}")
            if scales.dim() != 2 or scales.shape[1] != self.N or scales.shape[0] not in (1, self.K // 128):
                raise ValueError(f"fp8 Linear: scales [1, N] or [K/128, N], got {tuple(scales.shape)}")
            dev = scales.device
            scales = scales.to(torch.float32)
            if dev.type == "cuda":
                codes = codes.to(dev)
                perm = row_permutation(self.N, self.layout)
                if perm is not None:
                    pd = perm.to(dev)
                    codes, scales = codes[pd], scales[:, pd]
                self.wp = pack_fp8(codes.contiguous())
                self.fscales = scales.contiguous()
            else:
                self.w = fp8_dequant_ref(codes, scales)
            return
        if self.kind == "awq":
            q = awq["qint"]
            self.N, self.K = q.shape
            self.group = awq["group"]
            dev = awq["scales"].device
            perm = row_permutation(self.N, self.layout)
            scales, zeros = awq["scales"], awq["zeros"]
            if dev.type == "cuda":
                q = q.to(dev)
                if perm is not None:
                    pd = perm.to(dev)
                    q, scales, zeros = q[pd], scales[:, pd], zeros[:, pd]
                self.wp = pack_awq(q)
                self.scales = scales.to(torch.bfloat16).contiguous()
                self.zeros = (scales.float() * zeros.float()).to(torch.bfloat16).contiguous()
                if self.group == 128:
                    self.szp = pack_awq_sz(self.scales, self.zeros)
            else:
                self.w = ref.awq_dequant_ref(q, scales, zeros, self.group)
            return
        self.N, self.K = w.shape
        if w.is_cuda:
            perm = row_permutation(self.N, self.layout)
            self.wp = pack_weight(w[perm.to(w.device)] if perm is not None else w)
        else:
            self.w = w

    @classmethod
    def quantize_fp8(cls, w: torch.Tensor, bias: torch.Tensor | None = None, layout: str = "plain") -> "Linear":
        """Load-time per-output-channel FP8 quantization of a bf16 matrix [N, K]: s = amax_row / 448 (1 for
        an all-zero row), code = (w / s) rounded to e4m3fn."""
        wf = w.float()
        amax = wf.abs().amax(dim=1)
        s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        codes = (wf / s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        return cls(None, bias, fp8={"codes": codes, "scales": s[None].contiguous(), "layout": layout})

    @classmethod
    def quantize_mxfp4(cls, w: torch.Tensor, bias: torch.Tensor | None = None, layout: str = "plain") -> "Linear":
        """Load-time MXFP4 quantization of a matrix [N, K] (OCP Microscaling v1.0): per 32-wide K block
        e = floor(log2(amax)) - 2 + 127 (127 for a zero block; kept within 2..252), elements divided by
        2^(e-127), rounded to nearest-even on the e2m1 grid and saturated at +-6."""
        codes, scales = mxfp4_quantize(w)
        return cls(None, bias, mxfp4={"codes": codes, "scales": scales, "layout": layout})

    def fold_norm(self, gamma: torch.Tensor) -> bool:
        """Fold the preceding RMSNorm's weight into the packed matrix: W'[n,k] = W[n,k]*g[k].

        The fused GEMM then applies only the per-row scale rsqrt(mean(x^2)+eps) (deferred, in
        the epilogue) and streams no gamma bytes. GPU bf16 weights only; returns whether folded.
        """
        if self.kind != "dense" or self.wp is None or self.norm_gamma is not None:
            return False
        g = gamma.to(self.wp.device, torch.float32).reshape(1, self.K // 32, 4, 1, 8)
        self.wp.copy_((self.wp.float() * g).to(torch.bfloat16))
        self.norm_gamma = gamma.detach().clone()
        return True

    def _original_rows(self, w: torch.Tensor) -> torch.Tensor:
        """Undo the layout's row permutation of an unpacked [N, K] matrix."""
        perm = row_permutation(self.N, self.layout)
        if perm is None:
            return w
        out = torch.empty_like(w)
        out[perm.to(w.device)] = w
        return out

    @property
    def out_features(self) -> int:
        return self.N // 2 if self.layout == "silu" else self.N

    def dense_weight(self) -> torch.Tensor:
        """[N, K] in the ORIGINAL row order (references / checkpoint export)."""
        if self.w is not None:
            return self.w
        if self.kind == "awq":  # dequantised bf16 v * s - s * z (references)
            q = unpack_awq(self.wp, self.N, self.K)  # permuted row order, like scales / zeros
            g = torch.arange(self.K, device=q.device) // self.group
            w = (q.float() * self.scales.float()[g].t() - self.zeros.float()[g].t()).to(torch.bfloat16)
            return self._original_rows(w)
        if self.kind == "fp8":  # bf16(code * scale), the CPU Linear's matrix
            return self._original_rows(fp8_dequant_ref(unpack_fp8(self.wp, self.N, self.K), self.fscales))
        if self.kind == "mxfp4":  # bf16(value * 2^(e-127)), exact: the CPU Linear's matrix
            return self._original_rows(mxfp4_dequant_ref(unpack_mxfp4(self.wp, self.N, self.K),
                                                         unpack_mxfp4_scales(self.mscales, self.N, self.K)))
        w = unpack_weight(self.wp, self.N, self.K)
        if self.norm_gamma is not None:  # un-fold (approximate: W' was rounded to bf16)
            w = (w.float() / self.norm_gamma.to(w.device, torch.float32)[None]).to(torch.bfloat16)
        return self._original_rows(w)

    def nbytes(self) -> int:
        """Bytes a decode step streams."""
        if self.kind == "awq" and self.w is None:
            n = self.wp.numel() * 4 + self.scales.numel() * 4  # int4 + (s, s*z) bf16 per group
            return n + (self.szp.numel() * 2 if self.szp is not None else 0)
        if self.kind == "fp8" and self.w is None:
            return self.wp.numel() + self.fscales.numel() * 4  # codes + fp32 scales
        if self.kind == "mxfp4" and self.w is None:
            return self.wp.numel() + self.mscales.numel()  # two codes per byte + one e8m0 byte per 32
        t = self.wp if self.wp is not None else self.w
        return t.numel() * t.element_size()

