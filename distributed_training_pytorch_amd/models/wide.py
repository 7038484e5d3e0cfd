"""WideMLP: the ToyModel architecture (Linear + LeakyReLU stack, ``toy_model_and_data.py:8-25``)
at widths where the matmuls are real GEMMs -- every Linear runs through ``ops.gemm``:
the LDS-tiled MFMA GEMMs of ``csrc/gemm.hip`` / ``csrc/gemm_ph8.hip`` (bias +
activation fused into the epilogue, activation gradient fused into the input-gradient
GEMM); fp32 or bf16 compute.

Same ``layers.{2i}.{weight,bias}`` state-dict layout as ``ToyModel``; parameters
are views into one flat fp32 buffer, so ``FlatDDP`` all-reduces them as one
bucket list and checkpoints interchange with plain ``nn.Sequential`` MLPs.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.gemm import mlp


class WideMLP(nn.Module):
    def __init__(self, widths=(2, 1024, 1024, 1024, 1024, 1), slope: float = 0.01,
                 compute_dtype: torch.dtype = torch.float32, fp8_recipe: str = "current", fp8_amax_history: int = 16):
        super().__init__()
        if fp8_recipe not in ("current", "delayed"):
            raise ValueError(f"fp8_recipe must be 'current' or 'delayed', got {fp8_recipe!r}")
        self.fp8_recipe, self.fp8_amax_history = fp8_recipe, int(fp8_amax_history)
        if len(widths) < 2:
            raise ValueError("WideMLP needs at least an input and an output width")
        self.widths = tuple(int(w) for w in widths)
        self.slope = slope
        self.compute_dtype = compute_dtype
        mods: list[nn.Module] = []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2:
                mods.append(nn.LeakyReLU(slope))
        self.layers = nn.Sequential(*mods)
        self._flatten()

    def _flatten(self):
        ps = list(self.layers.parameters())
        flat = torch.empty(sum(p.numel() for p in ps), dtype=ps[0].dtype, device=ps[0].device)
        o = 0
        for p in ps:
            n = p.numel()
            flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat[o:o + n].view_as(p)
            o += n
        self._flat = flat

    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._flatten()
        return out

    def _fp8_state(self, weights):
        """The delayed-scaling state (``fp8_recipe='delayed'``), made on the first forward on the weights' device;
        a fresh one (re-seeded on its first step) after the module moved."""
        if self.fp8_recipe != "delayed" or self.compute_dtype != torch.float8_e4m3fn:
            return None
        st = getattr(self, "_fp8", None)
        if st is None or st.device != weights[0].device:
            from ..ops.fp8 import delayed_state_for

            st = self._fp8 = delayed_state_for(weights, self.fp8_amax_history)
        return st

    def linears(self) -> list[nn.Linear]:
        return [m for m in self.layers if isinstance(m, nn.Linear)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        lin = self.linears()
        ws = [m.weight for m in lin]
        return mlp(x, ws, [m.bias for m in lin], self.slope, self.compute_dtype, fp8_state=self._fp8_state(ws))

    def reference_forward(self, x: torch.Tensor) -> torch.Tensor:
        """Plain PyTorch forward of the same module tree (tests / stock baseline)."""
        return self.layers(x)
