"""Per-agent LoRA adapters on a shared base model.

An adapter is a PEFT-style directory: adapter_config.json (r, lora_alpha,
target_modules) + adapter_model.safetensors with tensors named
  base_model.model.model.layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight
  base_model.model.model.layers.{i}.mlp.{gate,up,down}_proj.lora_{A,B}.weight
A is [r, in], B is [out, r]; any subset of the seven projections may be
present, a missing one contributes zero.

The model keeps fused qkv_proj / gate_up GEMMs, so the loader stacks the
per-projection pairs: A along rank ([3r, K] for qkv), B block-diagonally
([N_q + 2 N_kv, 3r]) with the adapter scale lora_alpha / r folded in.
engine.lora_max_rank therefore bounds the ADAPTER's r, and the pool rank
is 3x that for qkv, 2x for gate_up, 1x for o / down; smaller ranks are
zero-padded.

LoraPool holds, per fused projection, A[L, S, R, K] and B[L, S, N, R]
(S = engine.lora_slots), allocated once: the hipGraph-captured decode
holds their addresses, so loading an adapter is an in-place copy_ into
slot s and freeing one zero-fills it. Slots are refcounted by adapter
path. Which slot a token row uses is a device int32 id (-1 = base model)
read by the BGMV kernels (ops.lora_apply).
"""

from __future__ import annotations

import os
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops

# fused projection -> the HF modules stacked into it, in output order
FUSED: Dict[str, Tuple[str, ...]] = {
    "qkv": ("q_proj", "k_proj", "v_proj"),
    "o": ("o_proj",),
    "gate_up": ("gate_proj", "up_proj"),
    "down": ("down_proj",),
}
_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn",
           "o_proj": "self_attn", "gate_proj": "mlp", "up_proj": "mlp",
           "down_proj": "mlp"}
KNOWN_MODULES = tuple(_PARENT)
KERNEL_MAX_R = 64  # ops.lora_shrink / lora_expand_add: R % 8 == 0, R <= 64


class LoraError(ValueError):
    pass


def adapter_key(path: str) -> str:
    """Canonical adapter identity (pool refcounts, prefix-sharing keys)."""
    return os.path.abspath(os.path.expanduser(path))


def read_adapter_config(path: str) -> Dict:
    """Parse and sanity-check adapter_config.json of an adapter directory."""
    from ..engine.base import AdapterNotFound, validate_adapter_dir
    try:
        return validate_adapter_dir(path)
    except AdapterNotFound as exc:
        raise LoraError(str(exc)) from exc


def check_max_rank(max_rank: int) -> None:
    if max_rank < 1 or 3 * max_rank > KERNEL_MAX_R:
        raise LoraError(
            f"engine.lora_max_rank={max_rank} unsupported: the fused qkv "
            f"projection stacks q, k and v along rank (pool R = 3 * max_rank, "
            f"rounded up to 8) and the BGMV kernels take R <= {KERNEL_MAX_R}")


def _pad8(n: int) -> int:
    return -(-n // 8) * 8


def proj_dims(cfg) -> Dict[str, Tuple[int, Tuple[int, ...]]]:
    """fused projection -> (K, per-module output sizes) for a LlamaConfig."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {
        "qkv": (H, (cfg.q_size, cfg.kv_size, cfg.kv_size)),
        "o": (cfg.q_size, (H,)),
        "gate_up": (H, (I, I)),
        "down": (I, (H,)),
    }


def pool_rank(proj: str, max_rank: int) -> int:
    return _pad8(len(FUSED[proj]) * max_rank)


def stack_pairs(pairs: Sequence[Optional[Tuple[torch.Tensor, torch.Tensor]]],
                out_sizes: Sequence[int], K: int, max_rank: int,
                scale: float, R: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stack per-module (A [r, K], B [out, r]) pairs of one fused projection
    into f32 (A_st [R, K], B_st [sum(out), R]): module j owns rank rows
    [j*max_rank, j*max_rank + r) of A_st and the matching block of B_st
    (block-diagonal), B carries `scale`. None = module not targeted."""
    R = R or _pad8(len(pairs) * max_rank)
    A_st = torch.zeros(R, K, dtype=torch.float32)
    B_st = torch.zeros(sum(out_sizes), R, dtype=torch.float32)
    n0 = 0
    for j, (pair, n) in enumerate(zip(pairs, out_sizes)):
        if pair is not None:
            A, B = pair
            r = A.size(0)
            A_st[j * max_rank:j * max_rank + r] = A.float()
            B_st[n0:n0 + n, j * max_rank:j * max_rank + r] = B.float() * scale
        n0 += n
    return A_st, B_st


def load_adapter(path: str, cfg, max_rank: int
                 ) -> List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]:
    """Load + validate an adapter against the base LlamaConfig. Returns,
    per layer, {fused projection: (A_st, B_st)} as stack_pairs built them
    (f32, CPU); projections the adapter does not touch are absent."""
    from safetensors.torch import load_file

    acfg = read_adapter_config(path)
    r = int(acfg["r"])
    if r < 1:
        raise LoraError(f"adapter {path!r}: r={r} is not a rank")
    if r > max_rank:
        raise LoraError(
            f"adapter {path!r}: r={r} exceeds engine.lora_max_rank={max_rank}")
    alpha = float(acfg.get("lora_alpha", r))
    scale = alpha / r
    targets = acfg.get("target_modules") or []
    if isinstance(targets, str):
        targets = [targets]
    unknown = sorted(set(targets) - set(KNOWN_MODULES))
    if unknown:
        raise LoraError(
            f"adapter {path!r}: unsupported target_modules {unknown} "
            f"(supported: {list(KNOWN_MODULES)})")
    st_p = os.path.join(adapter_key(path), "adapter_model.safetensors")
    if not os.path.exists(st_p):
        raise LoraError(f"adapter {path!r}: adapter_model.safetensors missing")
    sd = load_file(st_p)
    dims = proj_dims(cfg)
    mod_dims = {}
    for proj, mods in FUSED.items():
        K, outs = dims[proj]
        for m, n in zip(mods, outs):
            mod_dims[m] = (K, n)
    used = set()
    layers = []
    for i in range(cfg.n_layers):
        per_layer = {}
        for proj, mods in FUSED.items():
            K, outs = dims[proj]
            pairs = []
            for m in mods:
                base = f"base_model.model.model.layers.{i}.{_PARENT[m]}.{m}."
                ka, kb = base + "lora_A.weight", base + "lora_B.weight"
                if (ka in sd) != (kb in sd):
                    raise LoraError(f"adapter {path!r}: {base}* has only one "
                                    "of lora_A / lora_B")
                if ka not in sd:
                    pairs.append(None)
                    continue
                if targets and m not in targets:
                    raise LoraError(f"adapter {path!r}: tensors for {m} but "
                                    "it is not in target_modules")
                A, B = sd[ka], sd[kb]
                Km, n = mod_dims[m]
                if tuple(A.shape) != (r, Km) or tuple(B.shape) != (n, r):
                    raise LoraError(
                        f"adapter {path!r}: layer {i} {m} has A "
                        f"{tuple(A.shape)} / B {tuple(B.shape)}, base model "
                        f"{cfg.name} needs A {(r, Km)} / B {(n, r)}")
                used.update((ka, kb))
                pairs.append((A, B))
            if any(p is not None for p in pairs):
                per_layer[proj] = stack_pairs(pairs, outs, K, max_rank, scale)
        layers.append(per_layer)
    covered = sum(1 for per_layer in layers if per_layer)
    if covered not in (0, cfg.n_layers):
        raise LoraError(
            f"adapter {path!r}: tensors for {covered} layers, base model "
            f"{cfg.name} has {cfg.n_layers}")
    extra = sorted(set(sd) - used)
    if extra:
        raise LoraError(
            f"adapter {path!r}: {len(extra)} tensors do not belong to a "
            f"{cfg.n_layers}-layer {cfg.name} (first: {extra[0]})")
    return layers


@dataclass
class LoraContext:
    """What one forward needs to apply adapters: per-row slot ids on the
    device (decode and every device-fed path), or host-known segments
    [(slot, row_index_tensor)] (prefill: two plain matmuls per distinct
    adapter instead of re-reading A once per token). Rows in no segment /
    with id -1 are base-model or pad rows."""
    pool: "LoraPool"
    ids: Optional[torch.Tensor] = None
    segments: Optional[List[Tuple[int, torch.Tensor]]] = None

    def apply(self, layer: int, proj: str, y: torch.Tensor,
              x: torch.Tensor) -> None:
        """y += delta of this layer's fused projection, in place."""
        A, B = self.pool.pair(layer, proj)
        if self.segments is None:
            ops.lora_apply(y, x, A, B, self.ids)
            return
        for slot, rows in self.segments:
            v = x.index_select(0, rows).float() @ A[slot].float().t()
            d = v @ B[slot].float().t()
            y.index_copy_(0, rows,
                          (y.index_select(0, rows).float() + d).to(y.dtype))


class LoraPool:
    """Fixed device pool of adapter slots for one ModelInstance."""

    def __init__(self, cfg, slots: int, max_rank: int, device: str):
        check_max_rank(max_rank)
        if slots < 1:
            raise LoraError("LoraPool needs at least one slot")
        self.cfg = cfg
        self.slots = slots
        self.max_rank = max_rank
        self.device = device
        self._A: Dict[str, torch.Tensor] = {}
        self._B: Dict[str, torch.Tensor] = {}
        L = cfg.n_layers
        for proj, (K, outs) in proj_dims(cfg).items():
            R = pool_rank(proj, max_rank)
            self._A[proj] = torch.zeros(L, slots, R, K, dtype=torch.bfloat16,
                                        device=device)
            self._B[proj] = torch.zeros(L, slots, sum(outs), R,
                                        dtype=torch.bfloat16, device=device)
        self._lock = threading.Lock()
        self._slot_of: Dict[str, int] = {}
        self._refs: Dict[str, int] = {}
        self._free: List[int] = list(range(slots - 1, -1, -1))

    def pair(self, layer: int, proj: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(A [S, R, K], B [S, N, R]) views for one layer + projection."""
        return self._A[proj][layer], self._B[proj][layer]

    def acquire(self, path: str) -> int:
        """Slot of the adapter at `path`, loading it on first use. The
        copies are issued on the current stream — the one decode runs on
        — so later graph replays are ordered after them."""
        key = adapter_key(path)
        with self._lock:
            slot = self._slot_of.get(key)
            if slot is not None:
                self._refs[key] += 1
                return slot
            if not self._free:
                raise LoraError(
                    f"no free LoRA slot for adapter {path!r}: all "
                    f"{self.slots} slots (engine.lora_slots) hold adapters "
                    f"in use ({sorted(self._slot_of)})")
            layers = load_adapter(key, self.cfg, self.max_rank)  # may raise
            slot = self._free.pop()
            for i, per_layer in enumerate(layers):
                for proj, (A_st, B_st) in per_layer.items():
                    self._A[proj][i, slot].copy_(A_st.to(torch.bfloat16))
                    self._B[proj][i, slot].copy_(B_st.to(torch.bfloat16))
            if str(self.device).startswith("cuda"):
                # one sync, so a prefill on the side stream sees them too
                torch.cuda.current_stream().synchronize()
            self._slot_of[key] = slot
            self._refs[key] = 1
            return slot

    def release(self, path: str) -> None:
        """Drop one reference; the last one zero-fills and frees the slot."""
        key = adapter_key(path)
        with self._lock:
            if key not in self._refs:
                return
            self._refs[key] -= 1
            if self._refs[key] > 0:
                return
            slot = self._slot_of.pop(key)
            del self._refs[key]
            for proj in FUSED:
                self._A[proj][:, slot].zero_()
                self._B[proj][:, slot].zero_()
            self._free.append(slot)

    def resident(self) -> List[Dict]:
        with self._lock:
            return [{"adapter": k, "slot": s, "refcount": self._refs[k]}
                    for k, s in sorted(self._slot_of.items(),
                                       key=lambda kv: kv[1])]
