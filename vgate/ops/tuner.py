"""Start-up tuner of the medium / prefill GEMM decomposition, its plan encoding and plan cache."""
from __future__ import annotations

import hashlib
import json
import os

import torch

from ._native import PATH_MID, PATH_PREFILL, _dev_key, native, native_available
from .buffers import _per_device, workspace
from .packing import pack_weight


def _plan_bucket(plan: dict, M: int):
    """Smallest planned M >= M (a step's rows are padded up to its graph bucket), else None.
    Medium rows (M < 128) only take a medium bucket's plan (they are timed against another
    default path than the prefill buckets)."""
    keys = [k for k in plan if k >= M and (M >= 128 or k < 128)]
    return min(keys) if keys else None


# (tile code, K slices) candidates of the prefill kernels (csrc/kernels/gemm_prefill.hip
# launch_prefill_epi): 0 = the launcher's heuristic, 64 / 128 = 128 x 64 / 128 x 128 tiles,
# 256 = 256 x 128 3-deep ring, 768 / 1024 = the 4-phase 256 x 128 / 256 x 256 kernels
PREFILL_CANDIDATES = [(0, 0), (64, 0), (128, 0), (128, 2), (128, 4), (256, 0), (256, 4), (256, 6), (768, 0),
                      (768, 2), (768, 3), (768, 4), (768, 6), (1024, 0), (1024, 2), (1024, 3), (1024, 4),
                      (1024, 6), (1025, 0), (769, 0)]
# (1025 / 769: the persistent forms of the 4-phase 256 x 256 / 256 x 128 kernel — one block per CU,
# whole rounds of tiles + the last round K-split and met in-launch; gemm_prefill.hip
# gemm_prefill4sk_kernel)
# 128-row tiles on a 4-deep ring, one block per CU (128 x 128 / 128 x 64, 4 or 8 waves): timed for
# 64 < M <= 1024 only, where the grid of the 2-deep-ring tile is one or two partial rounds
# + the wide-N tiles 64 x 512 / 128 x 320 (gate_up at 320 / 448 rows: 245 / 224 blocks, 35 vs 44-64 us)
PREFILL_RING_CANDIDATES = ([(t, s) for t in (1280, 1281, 640, 641) for s in (0, 2, 3)]
                           + [(2560, 0), (2561, 0)])
# medium-M kernel (csrc/kernels/gemm_mid.hip, 16 < M <= 64) candidates, encoded as tile code
# MID_BASE - W (W tiles = waves per block) and K slices (0 = its heuristic)
MID_BASE = -10
MID_CANDIDATES = [(MID_BASE - w, s) for w in (4, 2) for s in (0, 2, 3, 4, 6, 8, 10, 12, 16)] + [(MID_BASE - 8, 0)]
_FLUSH: dict = {}


def _event_ms(run, n: int = 1) -> float:
    """Device time of ``n`` back-to-back ``run()`` calls, in ms."""
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(n):
        run()
    s1.record()
    s1.synchronize()
    return s0.elapsed_time(s1)


def _cold_timer(dev):
    """Event timer of one launch with the Infinity Cache flushed first: a 512 MiB read sweep evicts
    the weights a back-to-back repeat would find resident (gate_up's 55 MB fits the 256 MiB cache),
    so medium-M candidates are ranked by the cold-weight time they take inside a decode step."""
    buf = _per_device(_FLUSH, dev, lambda: torch.empty(512 * 2**20, dtype=torch.uint8, device=dev))
    C = native()

    def timed(run, iters):
        total = 0.0
        for _ in range(iters):
            C.prefetch(buf, 1024)
            total += _event_ms(run)
        return total / iters
    return timed


def _mid_code(cfg) -> int:
    """Waves per block of a medium-kernel plan entry, 0 for any other entry."""
    return MID_BASE - cfg[0] if cfg is not None and cfg[0] <= MID_BASE - 1 else 0


def _plan_kw(cfg, M: int) -> dict:
    """C.gemm keyword overrides of a plan entry (empty: the default path)."""
    if cfg is None or cfg == MEDIUM_DEFAULT or (cfg == (0, 0) and M >= 128):
        return {}
    w = _mid_code(cfg)
    if w:
        return dict(path=PATH_MID, waves=w, splitk=cfg[1])
    return dict(ntb=cfg[0], splitk=cfg[1], path=PATH_PREFILL)


MEDIUM_DEFAULT = (-1, -1)  # medium-M plan entry: keep the default (decode / tile kernel) path


# bump whenever the MEANING of a stored plan changes on the Python side (the _plan_kw encoding of a
# (tile, K slices) code, MID_BASE, the tuner margin): a cached plan set is keyed on this too
PLAN_FORMAT = 3  # 3: candidates timed with the layer's folded-norm row scale
TUNE_MARGIN = 0.05
LONG_M, LONG_MARGIN = 1024, 0.02  # the margin for M >= LONG_M buckets


def _gpu_packed(lins: list) -> list:
    """The Linears that hold a packed weight on a GPU (the ones the tuner can time)."""
    return [lin for lin in lins if getattr(lin, "wp", None) is not None and lin.wp.is_cuda]


def tune_prefill(lins: list, ms: list[int], iters: int = 5, margin: float = TUNE_MARGIN) -> dict:
    """Start-up measurement of the prefill GEMM decomposition per (N, K) shape and M bucket.

    The launcher's tile / K-split heuristic misses by up to 1.8x at mid M, where the grid of
    one tile shape needs a second partial round on 256 CUs and another's does not (Qwen2.5-1.5B
    gate_up at M = 384: 64 us heuristic vs 35 us for 128 x 128 tiles; down at M = 512: 56 vs
    40 us, profiles/r2_prefill_tile_sweep.log). Every candidate is timed on random operands of
    the layer's shape (plain epilogue, all candidates are exact kernels of the same product);
    the heuristic is kept unless a candidate beats it by more than ``margin``. The plan is
    shared by every Linear of the same shape (AWQ layers: the plan of their bf16 dequant scratch).

    Medium buckets (16 < M < 128: the mixed steps of a serving load, one prompt chunk beside the
    decode rows) are timed against the DEFAULT path at that M too (the K-split decode kernels /
    the LDS tile kernel, which stream the weights with one or two k-step groups in flight: a
    Qwen2.5-1.5B step with a 48-token prompt took 2.77 ms against 1.24 ms for pure decode,
    profiles/r3_mixed_step.log); the entry is :data:`MEDIUM_DEFAULT` unless a prefill
    decomposition beats that path by more than ``margin``.
    Returns {(N, K): {M: (tile, slices)}}."""
    cand = _gpu_packed(lins)
    if not cand or not native_available():
        return {}
    C = native()
    dev = cand[0].wp.device
    ws = workspace(dev)
    plans: dict = {}
    for lin in cand:
        key = (lin.N, lin.K)
        if key in plans:
            lin.prefill_plan = plans[key]
            continue
        plan = {}
        g = torch.Generator(device=dev)
        g.manual_seed(lin.N + lin.K)
        # AWQ / FP8 / MXFP4 layers run their long steps on a bf16 fragment-packed dequant scratch of the same shape
        # (_linear_awq_dequant / _linear_fp8_dequant / _linear_mxfp4_dequant): time a random bf16 matrix in that layout
        wp = lin.wp if lin.kind == "dense" else pack_weight(
            (torch.rand(lin.N, lin.K, device=dev, generator=g) * 2 - 1).bfloat16())
        # the folded RMSNorm's row scale as in the step (qkv / gate_up: the x^2 sums ride in the K loop
        # and cost some kernels up to ~30 % more than others — 128 x 320 tiles with four wave columns:
        # Qwen2.5-1.5B qkv at 448 rows 17.7 -> 22.9 us, profiles/r6_tuner_norm_timing.log)
        # (a QK-norm model's QKV projection is a plain-layout Linear that still takes the row scale: Linear.norm_in)
        nkw = (dict(rownorm=True, eps=1e-6)
               if lin.norm_gamma is not None or lin.layout in ("qkv", "silu") or getattr(lin, "norm_in", False) else {})
        for M in ms:
            x = torch.rand(M, lin.K, device=dev, generator=g).bfloat16()
            out = torch.empty(M, lin.N, dtype=torch.bfloat16, device=dev)
            times = {}
            # (cold-weight timing for M >= 128 too was measured: it picked slower down_proj plans at
            # M = 448 and the same gate_up tile, profiles/r4_prefill_step_timeline.log)
            cold = _cold_timer(dev) if M < 128 else None
            extra = MID_CANDIDATES if 16 < M <= 64 else PREFILL_RING_CANDIDATES if 64 < M <= 1024 else []
            for bn, sk in PREFILL_CANDIDATES + extra:
                def run():
                    C.gemm(x, wp, lin.N, lin.K, out, 0, ws=ws, **_plan_kw((bn, sk), M), **nkw)
                try:
                    run()
                except RuntimeError:
                    continue
                times[(bn, sk)] = cold(run, iters) if cold is not None else _event_ms(run, iters) / iters
            if (0, 0) not in times:
                continue
            best = min(times, key=times.get)
            if M < 128:
                # medium bucket: against the default path (M > 16 rows -> decode / tile kernels)
                def run_default():
                    C.gemm(x, wp, lin.N, lin.K, out, 0, ws=ws, **nkw)
                run_default()
                t_def = cold(run_default, iters)
                plan[M] = best if times[best] < (1.0 - margin) * t_def else MEDIUM_DEFAULT
                continue
            # long chunks: 100+ us launches time to ~1 %, so a 2 % win is kept (Llama-3-8B qkv_proj at
            # 2048 rows: split-K 6 + reduce 105 vs 111 us for the default grid sat on the 5 % edge)
            m_eff = margin if M < LONG_M else LONG_MARGIN
            plan[M] = best if times[best] < (1.0 - m_eff) * times[(0, 0)] else (0, 0)
        plans[key] = plan
        lin.prefill_plan = plan
    # the cache-flush buffer of the cold timer (512 MiB) is start-up scratch: give it back
    _FLUSH.pop(_dev_key(dev), None)
    torch.cuda.empty_cache()
    return plans


def _plan_cache_key(lins: list, ms: list[int]) -> str:
    """What a stored plan set was measured for: the device, the native build (size + mtime of the
    extension), the plan encoding (PLAN_FORMAT, TUNE_MARGIN) and every (N, K) shape x M bucket x
    candidate list — any change re-measures."""
    dev = lins[0].wp.device
    props = torch.cuda.get_device_properties(dev)
    so = getattr(native(), "__file__", "") or ""
    st = os.stat(so) if so and os.path.exists(so) else None
    shapes = sorted({(lin.N, lin.K, lin.kind) for lin in lins if getattr(lin, "wp", None) is not None})
    blob = json_dumps([PLAN_FORMAT, TUNE_MARGIN, LONG_M, LONG_MARGIN, props.name, props.multi_processor_count, st.st_size if st else 0,
                       int(st.st_mtime) if st else 0, shapes, sorted(ms), PREFILL_CANDIDATES, PREFILL_RING_CANDIDATES,
                       MID_CANDIDATES])
    return hashlib.sha1(blob.encode()).hexdigest()


def json_dumps(x) -> str:
    return json.dumps(x, sort_keys=True, default=str)


def load_plan_cache(path: str, key: str) -> dict | None:
    """Plans stored by :func:`save_plan_cache` under ``key``, or None."""
    try:
        with open(os.path.expanduser(path)) as f:
            d = json.load(f).get(key)
    except (OSError, ValueError):
        return None
    if not isinstance(d, dict):
        return None
    return {tuple(int(v) for v in nk.split(",")): {int(m): tuple(c) for m, c in plan.items()} for nk, plan in d.items()}


def save_plan_cache(path: str, key: str, plans: dict) -> None:
    """Persist measured plans under ``key`` (other keys in the file are kept; best effort)."""
    path = os.path.expanduser(path)
    try:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            d = {}
        d[key] = {f"{n},{k}": {str(m): list(c) for m, c in plan.items()} for (n, k), plan in plans.items()}
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump(d, f)
        os.replace(tmp, path)
    except OSError:
        pass


def tune_prefill_cached(lins: list, ms: list[int], cache: str | None) -> tuple[dict, bool]:
    """:func:`tune_prefill` behind a per-(device, build, shapes) plan file: a restart of the same
    engine on the same device skips the start-up measurement (~3,400 cache-flush launches for
    Qwen2.5-1.5B). Returns (plans, from_cache)."""
    cand = _gpu_packed(lins)
    if not cache or not cand or not native_available():
        return tune_prefill(lins, ms), False
    key = _plan_cache_key(cand, ms)
    plans = load_plan_cache(cache, key)
    if plans is not None:
        apply_prefill_plans(lins, plans)
        return plans, True
    plans = tune_prefill(lins, ms)
    save_plan_cache(cache, key, plans)
    return plans, False


def apply_prefill_plans(lins: list, plans: dict) -> None:
    """Give every Linear the plan measured for its (N, K) shape (plans from :func:`tune_prefill`,
    e.g. broadcast from TP rank 0)."""
    for lin in lins:
        plan = (plans or {}).get((lin.N, lin.K))
        if plan is not None:
            lin.prefill_plan = dict(plan)
