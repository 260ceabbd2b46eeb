"""Weight creation / loading for :class:`vgate.models.transformer.DecoderModel`.

* ``random_init``: seeded random weights generated directly on the device in
  kernel-ready (fragment-packed) form — the benchmark path (no checkpoints
  exist on this machine). Scales keep activations O(1) so numerics are sane.
* ``load_checkpoint``: HF safetensors (bf16/fp16/fp32, AWQ int4 GEMM format, FP8 e4m3 with block /
  per-channel / per-tensor weight scales, or MXFP4: packed e2m1 nibbles with e8m0 block-32 scales),
  sharded for the model's TP rank at load time (only this rank's slices are
  materialised on the GPU).
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import torch

from vgate import ops
from vgate.models.config import ModelArch

AWQ_ORDER = [0, 2, 4, 6, 1, 3, 5, 7]  # AutoAWQ GEMM nibble order within an int32
_FP8_DTYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz")
                    if hasattr(torch, n))


def _gen(device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def _randn(shape, std, g, device):
    return (torch.randn(shape, generator=g, device=device, dtype=torch.float32) * std).to(torch.bfloat16)


def _rand_awq(N, K, group, g, device, silu=False, layout="plain"):
    q = torch.randint(0, 16, (N, K), generator=g, device=device, dtype=torch.int32)
    target = 1.0 / math.sqrt(K)
    scales = torch.full((K // group, N), target / 4.61, device=device).to(torch.bfloat16)
    zeros = torch.full((K // group, N), 8.0, device=device).to(torch.bfloat16)
    return ops.Linear(None, awq={"qint": q, "scales": scales, "zeros": zeros, "group": group,
                                 "layout": "silu" if silu else layout})


QK_NORM_LO, QK_NORM_HI = 0.5, 4.0  # random-init range of the QK-norm weights (random_init)


def _rand_qk_norm(D, g, device):
    u = torch.rand(D, generator=g, device=device, dtype=torch.float32)
    return (QK_NORM_LO + (QK_NORM_HI - QK_NORM_LO) * u).to(torch.bfloat16)


def random_init(model, seed: int = 0) -> None:
    a: ModelArch = model.arch
    sh = model.shard
    dev = model.device
    g = _gen(dev, seed * 1000003 + sh.tp.rank)
    H, D = a.hidden_size, a.head_dim
    awq = model.quant == "awq"
    fp8 = model.quant == "fp8"
    mxfp4 = model.quant == "mxfp4"
    group = 128
    model.embed = _randn((sh.vocab, H), 0.02, g, dev)
    layers = []
    from vgate.models.transformer import LayerWeights
    q_out = (sh.hq + 2 * sh.hkv) * D
    # QK-norm archs: the projection keeps its natural rows (the norm's own kernel rotates), and the two
    # norm weights come from a generator of their own, after the layer's other draws: they are replicated,
    # so the stream must not depend on the TP rank, and every other preset's stream stays as it was.
    # Uniform in [QK_NORM_LO, QK_NORM_HI] per element: a wide, non-constant range makes attention sharp,
    # as trained Qwen3 norms do, and a dropped or misplaced norm visible in the tokens.
    qkv_layout = "plain" if a.qk_norm else "qkv"
    gn = _gen(dev, seed * 1000003 + 500009) if a.qk_norm else None
    for _ in range(a.num_layers):
        qkv_b = _randn((q_out,), 0.02, g, dev) if a.qkv_bias else None
        if awq and H % 128 == 0 and (sh.hq * D) % 128 == 0 and sh.inter % 128 == 0:
            qkv = _rand_awq(q_out, H, group, g, dev, layout=qkv_layout)
            qkv.bias = qkv_b
            o = _rand_awq(H, sh.hq * D, group, g, dev)
            gu = _rand_awq(2 * sh.inter, H, group, g, dev, silu=True)
            down = _rand_awq(H, sh.inter, group, g, dev)
        else:
            qkv = ops.Linear(_randn((q_out, H), 1 / math.sqrt(H), g, dev), bias=qkv_b, layout=qkv_layout)
            o = ops.Linear(_randn((H, sh.hq * D), 1 / math.sqrt(sh.hq * D * sh.tp.size), g, dev))
            gu = ops.Linear(_randn((2 * sh.inter, H), 1 / math.sqrt(H), g, dev), kind="silu")
            down = ops.Linear(_randn((H, sh.inter), 1 / math.sqrt(sh.inter * sh.tp.size), g, dev))
        if fp8:  # the dense branch's draws, quantized per output channel (embedding and LM head stay bf16)
            qkv = ops.Linear.quantize_fp8(qkv.dense_weight(), bias=qkv_b, layout=qkv_layout)
            o = ops.Linear.quantize_fp8(o.dense_weight())
            gu = ops.Linear.quantize_fp8(gu.dense_weight(), layout="silu")
            down = ops.Linear.quantize_fp8(down.dense_weight())
        if mxfp4:  # the dense branch's draws in OCP MX blocks of 32 (embedding and LM head stay bf16)
            qkv = ops.Linear.quantize_mxfp4(qkv.dense_weight(), bias=qkv_b, layout=qkv_layout)
            o = ops.Linear.quantize_mxfp4(o.dense_weight())
            gu = ops.Linear.quantize_mxfp4(gu.dense_weight(), layout="silu")
            down = ops.Linear.quantize_mxfp4(down.dense_weight())
        qn, kn = (_rand_qk_norm(D, gn, dev), _rand_qk_norm(D, gn, dev)) if a.qk_norm else (None, None)
        layers.append(LayerWeights(
            in_norm=torch.ones(H, dtype=torch.bfloat16, device=dev), qkv=qkv, o=o,
            post_norm=torch.ones(H, dtype=torch.bfloat16, device=dev), gate_up=gu, down=down,
            q_norm=qn, k_norm=kn))
        if awq and dev.type == "cuda":
            torch.cuda.empty_cache()
    model.layers = layers
    model.final_norm = torch.ones(H, dtype=torch.bfloat16, device=dev)
    if a.tie_embeddings:
        model.lm_head = ops.Linear(model.embed)
    else:
        model.lm_head = ops.Linear(_randn((sh.vocab, H), 1 / math.sqrt(H), g, dev))


# ------------------------------------------------------------------ checkpoints
class _SafeTensorIndex:
    def __init__(self, path: Path):
        from safetensors import safe_open
        files = sorted(path.glob("*.safetensors")) if path.is_dir() else [path]
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {path}")
        self._handles = {}
        self._where = {}
        for f in files:
            h = safe_open(str(f), framework="pt", device="cpu")
            self._handles[str(f)] = h
            for k in h.keys():
                self._where[k] = str(f)

    def has(self, k: str) -> bool:
        return k in self._where

    def get(self, k: str) -> torch.Tensor:
        return self._handles[self._where[k]].get_tensor(k)

    def get_slice(self, k: str):
        return self._handles[self._where[k]].get_slice(k)


def unpack_awq_int32(packed: torch.Tensor) -> torch.Tensor:
    """AutoAWQ GEMM packing: [rows, cols/8] int32 -> [rows, cols] int (0..15)."""
    rows, c8 = packed.shape
    shifts = torch.tensor([4 * i for i in range(8)], dtype=torch.int32)
    vals = (packed.unsqueeze(-1) >> shifts) & 0xF  # nibble i
    # nibble i holds logical column AWQ_ORDER[i]
    out = torch.empty_like(vals)
    out[..., AWQ_ORDER] = vals
    return out.reshape(rows, c8 * 8)


def pack_awq_int32(q: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`unpack_awq_int32` (used by tests to build AWQ fixtures)."""
    rows, cols = q.shape
    v = q.reshape(rows, cols // 8, 8).to(torch.int64)[..., AWQ_ORDER]
    shifts = torch.tensor([4 * i for i in range(8)], dtype=torch.int64)
    w = (v << shifts).sum(-1)
    w = torch.where(w >= 2**31, w - 2**32, w)
    return w.to(torch.int32)


def _rows(t: torch.Tensor, a: int, b: int) -> torch.Tensor:
    return t[a:b]


def load_checkpoint(model, path: str) -> None:
    """Load an HF Qwen2 / Qwen3 / Llama checkpoint (safetensors) for this TP rank."""
    a: ModelArch = model.arch
    sh = model.shard
    dev = model.device
    root = Path(path)
    idx = _SafeTensorIndex(root)
    D, H = a.head_dim, a.hidden_size
    qcfg = {}
    if (root / "config.json").exists():
        qcfg = json.loads((root / "config.json").read_text()).get("quantization_config", {}) or {}
    group = int(qcfg.get("group_size", 128))

    def dense(name: str) -> torch.Tensor:
        t = idx.get(name)
        if t.dtype in _FP8_DTYPES:
            raise ValueError(f"{name}: {t.dtype} tensor where a bf16 / fp16 / fp32 one is expected")
        return t.to(torch.bfloat16)

    want_fp8 = model.quant == "fp8"
    block = qcfg.get("weight_block_size")

    def is_fp8(prefix: str) -> bool:
        return idx.has(prefix + ".weight") and idx.get_slice(prefix + ".weight").get_dtype().upper().startswith("F8")

    def fp8_parts(prefix: str, rows=None, ks=None):
        """(codes uint8 [N, K], scales fp32 [G, N], G = 1 or K / 128) of an fp8 projection, restricted to
        output rows [rows) or input columns [ks). The stored scale multiplies the code; activation
        scales (input_scale) are ignored: W8A16."""
        w = idx.get(prefix + ".weight")
        if w.dtype != torch.float8_e4m3fn:
            raise ValueError(f"{prefix}.weight: {w.dtype} is not supported (FP8 weights must be float8_e4m3fn)")
        N, K = w.shape
        codes = w.view(torch.uint8)
        if idx.has(prefix + ".weight_scale_inv"):
            if block is None or list(block) != [128, 128]:
                raise ValueError(f"{prefix}: block-scaled FP8 needs quantization_config.weight_block_size == "
                                 f"[128, 128], got {block}")
            s = idx.get(prefix + ".weight_scale_inv").float()
            if tuple(s.shape) != ((N + 127) // 128, (K + 127) // 128) or K % 128:
                raise ValueError(f"{prefix}.weight_scale_inv: shape {tuple(s.shape)} does not match 128 x 128 blocks "
                                 f"of a [{N}, {K}] weight with K % 128 == 0")
            scales = s.repeat_interleave(128, dim=0)[:N].t().contiguous()  # [K/128, N]
        elif idx.has(prefix + ".weight_scale"):
            s = idx.get(prefix + ".weight_scale").float()
            if s.numel() == 1:
                scales = s.reshape(1, 1).expand(1, N).contiguous()
            elif s.numel() == N and s.dim() <= 2 and s.shape[0] == N:
                scales = s.reshape(1, N).contiguous()
            else:
                raise ValueError(f"{prefix}.weight_scale: shape {tuple(s.shape)} is not [], [1], [N] or [N, 1]")
        else:
            raise ValueError(f"{prefix}: float8 weight without weight_scale_inv / weight_scale")
        if rows is not None:
            codes, scales = codes[rows[0]:rows[1]], scales[:, rows[0]:rows[1]]
        if ks is not None:
            if scales.shape[0] > 1:
                if ks[0] % 128 or ks[1] % 128:
                    raise ValueError(f"{prefix}: a TP shard's k-range [{ks[0]}, {ks[1]}) must be a multiple of the "
                                     f"128-wide scale blocks")
                scales = scales[ks[0] // 128: ks[1] // 128]
            codes = codes[:, ks[0]:ks[1]]
        return codes.contiguous(), scales.contiguous()

    def make_fp8(parts, layout="plain", bias=None):
        """One Linear from the row-wise concatenation of (codes, scales) parts."""
        K = parts[0][0].shape[1]
        if K % 128:
            raise ValueError(f"FP8 Linear: K = {K} of this rank's shard is not a multiple of 128")
        G = max(s.shape[0] for _, s in parts)
        codes = torch.cat([c for c, _ in parts])
        scales = torch.cat([s.expand(G, -1) if s.shape[0] != G else s for _, s in parts], dim=1)
        return ops.Linear(None, bias, fp8={"codes": codes, "scales": scales.contiguous().to(dev), "layout": layout})

    def maybe_fp8(w: torch.Tensor, **kw):
        """A dense matrix of this rank: bf16 Linear, or quantized at load under ``quantization: fp8`` /
        ``quantization: mxfp4``."""
        if want_fp8:
            return ops.Linear.quantize_fp8(w.to(dev), **kw)
        if model.quant == "mxfp4":
            return ops.Linear.quantize_mxfp4(w.to(dev), **kw)
        return ops.Linear(w.to(dev), **kw)

    def is_mxfp4(prefix: str) -> bool:
        if not idx.has(prefix + ".weight"):
            return False
        dt = idx.get_slice(prefix + ".weight").get_dtype().upper()
        return dt == "U8" or dt.startswith("F4")

    def mxfp4_parts(prefix: str, rows=None, ks=None):
        """(codes uint8 [N, K] one nibble value per byte, scales uint8 [N, K/32]) of an MXFP4 projection:
        ``weight`` uint8 [N, K/2] with element 2i in the low nibble of byte i, ``weight_scale`` e8m0 bytes
        [N, K/32]; restricted to output rows [rows) or input columns [ks). Scale bytes are validated here so
        the message carries the tensor's name; activation-quantization entries (input_scale) are ignored: W4A16."""
        w = idx.get(prefix + ".weight")
        if w.dtype != torch.uint8:  # torch.float4_e2m1fn_x2, where the installed safetensors yields it
            w = w.view(torch.uint8)
        if w.dim() != 2:
            raise ValueError(f"{prefix}.weight: MXFP4 codes must be [N, K/2], got {tuple(w.shape)}")
        N, K = w.shape[0], 2 * w.shape[1]
        if not idx.has(prefix + ".weight_scale"):
            raise ValueError(f"{prefix}.weight: packed 4-bit weight without {prefix}.weight_scale")
        s = idx.get(prefix + ".weight_scale")
        if s.dtype != torch.uint8:
            if s.element_size() != 1:
                raise ValueError(f"{prefix}.weight_scale: {s.dtype} is not e8m0 (uint8 / float8_e8m0fnu)")
            s = s.view(torch.uint8)
        if K % 128:
            raise ValueError(f"{prefix}.weight: K = {K} is not a multiple of 128")
        if tuple(s.shape) != (N, K // 32):
            raise ValueError(f"{prefix}.weight_scale: shape {tuple(s.shape)} does not match [N, K/32] = "
                             f"[{N}, {K // 32}] of the weight")
        codes = torch.stack([w & 0xF, w >> 4], dim=-1).reshape(N, K)
        s = ops.packing.mxfp4_check_scales(codes, s, prefix + ".weight_scale")
        if rows is not None:
            codes, s = codes[rows[0]:rows[1]], s[rows[0]:rows[1]]
        if ks is not None:
            if ks[0] % 128 or ks[1] % 128:
                raise ValueError(f"{prefix}.weight: a TP shard's k-range [{ks[0]}, {ks[1]}) must be a multiple of 128")
            codes, s = codes[:, ks[0]:ks[1]], s[:, ks[0] // 32: ks[1] // 32]
        return codes.contiguous(), s.contiguous()

    def make_mxfp4(parts, layout="plain", bias=None):
        """One Linear from the row-wise concatenation of (codes, scales) parts."""
        codes = torch.cat([c for c, _ in parts])
        scales = torch.cat([s_ for _, s_ in parts])
        return ops.Linear(None, bias, mxfp4={"codes": codes, "scales": scales.to(dev), "layout": layout})

    def is_awq(prefix: str) -> bool:
        return idx.has(prefix + ".qweight")

    def awq_rows(prefix: str, row_ranges):
        """Return (qint [N, K], scales [K/g, N], zeros [K/g, N]) restricted to output rows."""
        qw = unpack_awq_int32(idx.get(prefix + ".qweight"))  # [K, N]
        qz = unpack_awq_int32(idx.get(prefix + ".qzeros"))   # [K/g, N]
        sc = idx.get(prefix + ".scales").to(torch.bfloat16)  # [K/g, N]
        cols = torch.cat([torch.arange(s, e) for s, e in row_ranges])
        return qw[:, cols].t().contiguous(), sc[:, cols].contiguous(), qz[:, cols].to(torch.bfloat16).contiguous()

    def awq_cols(prefix: str, k0: int, k1: int):
        qw = unpack_awq_int32(idx.get(prefix + ".qweight"))[k0:k1]
        qz = unpack_awq_int32(idx.get(prefix + ".qzeros"))[k0 // group:k1 // group]
        sc = idx.get(prefix + ".scales").to(torch.bfloat16)[k0 // group:k1 // group]
        return qw.t().contiguous(), sc.contiguous(), qz.to(torch.bfloat16).contiguous()

    def make_awq(t, silu=False, layout="plain"):
        q, s, z = t
        return ops.Linear(None, awq={"qint": q, "scales": s.to(dev), "zeros": z.to(dev), "group": group,
                                     "layout": "silu" if silu else layout})

    qkv_layout = "plain" if a.qk_norm else "qkv"  # QK-norm: natural rows, see random_init
    qa, qb = sh.q_head0 * D, (sh.q_head0 + sh.hq) * D
    ka, kb = a.q_size + sh.kv_head0 * D, a.q_size + (sh.kv_head0 + sh.hkv) * D
    va, vb = a.q_size + a.kv_size + sh.kv_head0 * D, a.q_size + a.kv_size + (sh.kv_head0 + sh.hkv) * D
    from vgate.models.transformer import LayerWeights
    layers = []
    for i in range(a.num_layers):
        p = f"model.layers.{i}"
        att, mlp = p + ".self_attn", p + ".mlp"
        bias = None
        if a.qkv_bias and idx.has(att + ".q_proj.bias"):
            full_b = torch.cat([dense(att + ".q_proj.bias"), dense(att + ".k_proj.bias"), dense(att + ".v_proj.bias")])
            bias = torch.cat([full_b[qa:qb], full_b[ka:kb], full_b[va:vb]]).to(dev)
        if is_awq(att + ".q_proj"):
            q = awq_rows(att + ".q_proj", [(qa, qb)])
            k = awq_rows(att + ".k_proj", [(ka - a.q_size, kb - a.q_size)])
            v = awq_rows(att + ".v_proj", [(va - a.q_size - a.kv_size, vb - a.q_size - a.kv_size)])
            qkv = make_awq((torch.cat([q[0], k[0], v[0]]), torch.cat([q[1], k[1], v[1]], 1),
                            torch.cat([q[2], k[2], v[2]], 1)), layout=qkv_layout)
            qkv.bias = bias
            o = make_awq(awq_cols(att + ".o_proj", qa, qb))
            g_ = awq_rows(mlp + ".gate_proj", [(sh.inter0, sh.inter0 + sh.inter)])
            u_ = awq_rows(mlp + ".up_proj", [(sh.inter0, sh.inter0 + sh.inter)])
            gu = make_awq((torch.cat([g_[0], u_[0]]), torch.cat([g_[1], u_[1]], 1), torch.cat([g_[2], u_[2]], 1)),
                          silu=True)
            down = make_awq(awq_cols(mlp + ".down_proj", sh.inter0, sh.inter0 + sh.inter))
        elif is_mxfp4(att + ".q_proj"):
            qkv = make_mxfp4([mxfp4_parts(att + ".q_proj", rows=(qa, qb)),
                              mxfp4_parts(att + ".k_proj", rows=(ka - a.q_size, kb - a.q_size)),
                              mxfp4_parts(att + ".v_proj", rows=(va - a.q_size - a.kv_size, vb - a.q_size - a.kv_size))],
                             layout=qkv_layout, bias=bias)
            o = make_mxfp4([mxfp4_parts(att + ".o_proj", ks=(qa, qb))])
            gu = make_mxfp4([mxfp4_parts(mlp + ".gate_proj", rows=(sh.inter0, sh.inter0 + sh.inter)),
                             mxfp4_parts(mlp + ".up_proj", rows=(sh.inter0, sh.inter0 + sh.inter))], layout="silu")
            down = make_mxfp4([mxfp4_parts(mlp + ".down_proj", ks=(sh.inter0, sh.inter0 + sh.inter))])
        elif is_fp8(att + ".q_proj"):
            qkv = make_fp8([fp8_parts(att + ".q_proj", rows=(qa, qb)),
                            fp8_parts(att + ".k_proj", rows=(ka - a.q_size, kb - a.q_size)),
                            fp8_parts(att + ".v_proj", rows=(va - a.q_size - a.kv_size, vb - a.q_size - a.kv_size))],
                           layout=qkv_layout, bias=bias)
            o = make_fp8([fp8_parts(att + ".o_proj", ks=(qa, qb))])
            gu = make_fp8([fp8_parts(mlp + ".gate_proj", rows=(sh.inter0, sh.inter0 + sh.inter)),
                           fp8_parts(mlp + ".up_proj", rows=(sh.inter0, sh.inter0 + sh.inter))], layout="silu")
            down = make_fp8([fp8_parts(mlp + ".down_proj", ks=(sh.inter0, sh.inter0 + sh.inter))])
        else:
            wq = dense(att + ".q_proj.weight")[qa:qb]
            wk = dense(att + ".k_proj.weight")[ka - a.q_size: kb - a.q_size]
            wv = dense(att + ".v_proj.weight")[va - a.q_size - a.kv_size: vb - a.q_size - a.kv_size]
            qkv = maybe_fp8(torch.cat([wq, wk, wv]), bias=bias, layout=qkv_layout)
            o = maybe_fp8(dense(att + ".o_proj.weight")[:, qa:qb].contiguous())
            wg = dense(mlp + ".gate_proj.weight")[sh.inter0: sh.inter0 + sh.inter]
            wu = dense(mlp + ".up_proj.weight")[sh.inter0: sh.inter0 + sh.inter]
            gu = maybe_fp8(torch.cat([wg, wu]), layout="silu")
            down = maybe_fp8(dense(mlp + ".down_proj.weight")[:, sh.inter0: sh.inter0 + sh.inter].contiguous())
        qn = kn = None
        if a.qk_norm:  # [head_dim] each, shared by every head: replicated on every TP rank
            missing = [k for k in (att + ".q_norm.weight", att + ".k_norm.weight") if not idx.has(k)]
            if missing:
                raise ValueError(f"{root}: the architecture has QK-norm (model_type qwen3) but the checkpoint "
                                 f"lacks {missing}")
            qn, kn = dense(att + ".q_norm.weight").to(dev), dense(att + ".k_norm.weight").to(dev)
            if qn.numel() != D or kn.numel() != D:
                raise ValueError(f"{att}: q_norm / k_norm must have head_dim = {D} elements")
        layers.append(LayerWeights(dense(p + ".input_layernorm.weight").to(dev), qkv, o,
                                   dense(p + ".post_attention_layernorm.weight").to(dev), gu, down, qn, kn))
    model.layers = layers
    emb = dense("model.embed_tokens.weight")
    pad = sh.vocab_padded - emb.shape[0]
    if pad > 0:
        emb = torch.cat([emb, torch.zeros(pad, H, dtype=emb.dtype)])
    model.embed = emb[sh.vocab0: sh.vocab0 + sh.vocab].contiguous().to(dev)
    model.final_norm = dense("model.norm.weight").to(dev)
    if a.tie_embeddings or not idx.has("lm_head.weight"):
        model.lm_head = ops.Linear(model.embed)
    else:
        lm = dense("lm_head.weight")
        if pad > 0:
            lm = torch.cat([lm, torch.zeros(pad, H, dtype=lm.dtype)])
        model.lm_head = ops.Linear(lm[sh.vocab0: sh.vocab0 + sh.vocab].contiguous().to(dev))


def save_checkpoint(model, path: str) -> None:
    """Write a TP=1 dense model as HF-layout safetensors (fast restart / tests)."""
    from safetensors.torch import save_file
    a = model.arch
    assert model.tp.size == 1
    out = {"model.embed_tokens.weight": model.embed[: a.vocab_size].cpu(), "model.norm.weight": model.final_norm.cpu()}
    for i, L in enumerate(model.layers):
        p = f"model.layers.{i}"
        w = L.qkv.dense_weight().cpu()
        out[p + ".self_attn.q_proj.weight"] = w[: a.q_size].contiguous()
        out[p + ".self_attn.k_proj.weight"] = w[a.q_size: a.q_size + a.kv_size].contiguous()
        out[p + ".self_attn.v_proj.weight"] = w[a.q_size + a.kv_size:].contiguous()
        if L.qkv.bias is not None:
            b = L.qkv.bias.cpu()
            out[p + ".self_attn.q_proj.bias"] = b[: a.q_size].contiguous()
            out[p + ".self_attn.k_proj.bias"] = b[a.q_size: a.q_size + a.kv_size].contiguous()
            out[p + ".self_attn.v_proj.bias"] = b[a.q_size + a.kv_size:].contiguous()
        out[p + ".self_attn.o_proj.weight"] = L.o.dense_weight().cpu().contiguous()
        gu = L.gate_up.dense_weight().cpu()
        I = gu.shape[0] // 2
        out[p + ".mlp.gate_proj.weight"] = gu[:I].contiguous()
        out[p + ".mlp.up_proj.weight"] = gu[I:].contiguous()
        out[p + ".mlp.down_proj.weight"] = L.down.dense_weight().cpu().contiguous()
        out[p + ".input_layernorm.weight"] = L.in_norm.cpu()
        out[p + ".post_attention_layernorm.weight"] = L.post_norm.cpu()
        if L.q_norm is not None:
            out[p + ".self_attn.q_norm.weight"] = L.q_norm.cpu()
            out[p + ".self_attn.k_norm.weight"] = L.k_norm.cpu()
    if not a.tie_embeddings:
        out["lm_head.weight"] = model.lm_head.dense_weight()[: a.vocab_size].cpu().contiguous()
    Path(path).mkdir(parents=True, exist_ok=True)
    save_file(out, str(Path(path) / "model.safetensors"))
    cfg = {"model_type": a.family, "hidden_size": a.hidden_size, "num_hidden_layers": a.num_layers,
           "num_attention_heads": a.num_heads, "num_key_value_heads": a.num_kv_heads,
           "intermediate_size": a.intermediate_size, "vocab_size": a.vocab_size, "rms_norm_eps": a.rms_eps,
           "rope_theta": a.rope_theta, "tie_word_embeddings": a.tie_embeddings,
           "max_position_embeddings": a.max_position, "head_dim": a.head_dim,
           "bos_token_id": a.bos_token_id, "eos_token_id": list(a.eos_token_ids)}
    if a.rope_scaling:
        cfg["rope_scaling"] = a.rope_scaling
    (Path(path) / "config.json").write_text(json.dumps(cfg, indent=1))
