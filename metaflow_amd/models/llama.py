"""Llama-3 architecture on the metaflow_amd HIP kernel library.

BASELINE config 3: the @parallel Llama-3-8B bf16 train step. All hot ops
are hand-written gfx950 HIP (ops.attention / rmsnorm / rope / swiglu /
cross_entropy); plain GEMMs go through torch.matmul -> hipBLASLt. Weights
random-init (no network for checkpoints), bf16.
"""

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import kernels as K
from .generate import generate
from .kv_cache import KVCache, PagedKVCache, PagedSlotView  # noqa: F401


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    max_seq_len: int = 8192
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    tie_embeddings: bool = False
    # fp8=True runs the decoder projections' FORWARD GEMMs in OCP E4M3
    # (delayed scaling, bf16 backward — ops/fp8.py); lm_head stays bf16.
    # fp8_bwd=True additionally runs dgrad/wgrad in E4M3 (delayed-scaled
    # dy) — the full-fp8 rung; watch loss quality
    fp8: bool = False
    fp8_bwd: bool = False
    # recompute=True checkpoints each decoder layer's activations
    # (recomputed in backward): activation memory drops from O(layers)
    # to O(1) layers — the knob that fits 70B/long-seq training
    recompute: bool = False

    @classmethod
    def llama3_8b(cls):
        return cls()

    @classmethod
    def llama3_70b(cls):
        return cls(hidden_size=8192, intermediate_size=28672, num_layers=80,
                   num_heads=64, num_kv_heads=8)

    @classmethod
    def tiny(cls, vocab=1024, seq=256):
        """CPU-testable config."""
        return cls(vocab_size=vocab, hidden_size=256, intermediate_size=688,
                   num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128,
                   max_seq_len=seq)


class Linear(nn.Module):
    """Bias-free bf16 linear -> hipBLASLt GEMM (offline-tuned solution
    indices where the shape is in ops/gemm_table.json; heuristic
    otherwise)."""

    def __init__(self, din, dout, dtype=torch.bfloat16):
        super().__init__()
        self.weight = nn.Parameter(
            torch.empty(dout, din, dtype=dtype))

    def forward(self, x):
        from ..ops.gemm import tuned_linear

        return tuned_linear(x, self.weight)


#: rows of x up to which a quantised projection takes the stream kernel:
#: at 8B geometry it beat the dequantising fallback on all five projections
#: at 64 and 128 rows (two passes over the weights); at 256 it lost on
#: gate|up and on the four layer projections together (docs/KERNELS.md,
#: "FP8 dense weights")
STREAM_MAX_ROWS = 128


class Fp8WeightLinear(nn.Module):
    """A bias-free linear with weight-only FP8 weights: E4M3 bytes
    ``weight8`` [out, in] and one fp32 ``scale`` per output row
    (K.moe_quant_weight), held as buffers, so state_dict round-trips and
    there is nothing to train. Up to STREAM_MAX_ROWS rows of x (decode) the
    bytes are streamed as they are (K.linear_w8); above (prefill) they are
    dequantised to a bf16 copy that lives for the call and go through the
    bf16 GEMM. ``swiglu(x)`` is the same for a packed gate|up weight and
    returns silu(gate) * up."""

    def __init__(self, din, dout, device=None):
        super().__init__()
        self.register_buffer("weight8", torch.zeros(
            dout, din, dtype=torch.float8_e4m3fn, device=device))
        self.register_buffer("scale", torch.ones(
            dout, dtype=torch.float32, device=device))

    @classmethod
    def from_linear(cls, linear):
        w = linear.weight
        q = cls(w.size(1), w.size(0), device=w.device)
        w8, scale = K.moe_quant_weight(w)
        q.weight8.copy_(w8)
        q.scale.copy_(scale)
        return q

    def _streams(self, x):
        return x.numel() // x.size(-1) <= STREAM_MAX_ROWS

    def _dense(self, x):
        from ..ops.gemm import tuned_linear

        return tuned_linear(x, K.linear_dequant(self.weight8, self.scale))

    def forward(self, x):
        if self._streams(x):
            return K.linear_w8(x, self.weight8, self.scale)
        return self._dense(x)

    def swiglu(self, x):
        if self._streams(x):
            return K.linear_w8(x, self.weight8, self.scale, swiglu=True)
        return K.swiglu_fused(self._dense(x))


class RMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, dtype=torch.bfloat16))
        self.eps = eps

    def forward(self, x):
        return K.rmsnorm(x, self.weight, self.eps)


def rope_rows(x, c, s):
    """Half-rotation RoPE with a per-BATCH position row: x [B,Hh,1,D],
    c/s [B, D/2] (each slot's own position — the batched-decode case the
    positional kernel's single-offset layout can't express)."""
    B, _hh, _one, D = x.shape
    half = D // 2
    c = c.view(B, 1, 1, half).float()
    s = s.view(B, 1, 1, half).float()
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


class _NoCache(object):
    """Attends over the fresh K/V where there is no cache, through the
    cache views' ``attend`` signature: flash attention, or the xGMI ring
    (parallel/ring_attention.py) for a context-parallel group."""

    def __init__(self, cp_group=None):
        self.cp_group = cp_group

    def attend(self, layer_idx, q, k, v, S, scale):
        if self.cp_group is None:
            return K.attention(q, k, v)
        from ..parallel.ring_attention import ring_attention

        return ring_attention(q, k, v, group=self.cp_group)


no_cache = _NoCache()


class DecoderLayer(nn.Module):
    """Fused projections: one QKV GEMM (the narrow separate K/V GEMMs are
    inefficient on MFMA) and one gate|up GEMM feeding the fused-layout
    SwiGLU kernel (no slice copies; its backward emits d_gateup directly).
    RoPE runs on the [B,H,S,D] layout the attention kernel consumes, so
    the transpose copy after the QKV split is the only data movement."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        h, hd = cfg.hidden_size, cfg.head_dim
        if cfg.fp8:
            import functools

            from ..ops.fp8 import Fp8Linear

            Lin = functools.partial(Fp8Linear, fp8_bwd=cfg.fp8_bwd)
        else:
            Lin = Linear
        self.qkv_proj = Lin(
            h, (cfg.num_heads + 2 * cfg.num_kv_heads) * hd)
        self.input_norm = RMSNorm(h, cfg.rms_eps)
        self.o_proj = Lin(cfg.num_heads * hd, h)
        self.post_norm = RMSNorm(h, cfg.rms_eps)
        self.gate_up_proj = Lin(h, 2 * cfg.intermediate_size)
        self.down_proj = Lin(cfg.intermediate_size, h)
        self.scale = 1.0 / math.sqrt(hd)

    def _block(self, res, pending, rope_qkv, cos, sin, view, layer_idx):
        """The layer body. Carries (residual_stream, pending_branch):
        every residual add fuses with the next RMSNorm (K.add_rmsnorm).
        `pending` is the previous layer's un-added MLP output (None for
        layer 0). ``rope_qkv(qkv, cos, sin, nq, nkv)`` gives the roped
        q, k, v in [B,H,S,D]; ``view`` attends."""
        cfg = self.cfg
        B, S, _ = res.shape
        hd = cfg.head_dim
        nq = cfg.num_heads
        res, y = K.add_rmsnorm(res, pending, self.input_norm.weight,
                               self.input_norm.eps)
        q, k, v = rope_qkv(self.qkv_proj(y), cos, sin, nq, cfg.num_kv_heads)
        o = view.attend(layer_idx, q, k, v, S, self.scale)
        o = o.transpose(1, 2).reshape(B, S, nq * hd)
        res, y = K.add_rmsnorm(res, self.o_proj(o), self.post_norm.weight,
                               self.post_norm.eps)
        if isinstance(self.gate_up_proj, Fp8WeightLinear):
            h = self.gate_up_proj.swiglu(y)
        else:
            h = K.swiglu_fused(self.gate_up_proj(y))
        pending = self.down_proj(h)
        return res, pending

    def _rope_qkv_rows(self, qkv, c_rows, s_rows, nq, nkv):
        """K.rope_qkv's counterpart for the batched decode step: qkv
        [B, 1, (nq+2*nkv)*hd] as heads [B, H, 1, hd], q and k rotated by
        each slot's own table row."""
        hd = self.cfg.head_dim
        q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
        q = q.view(-1, 1, nq, hd).transpose(1, 2)
        k = k.view(-1, 1, nkv, hd).transpose(1, 2)
        v = v.view(-1, 1, nkv, hd).transpose(1, 2)
        return rope_rows(q, c_rows, s_rows), rope_rows(k, c_rows, s_rows), v

    def forward(self, res, pending, cos_t, sin_t, cp_group=None,
                cache=None, layer_idx=0):
        """One fused kernel does the QKV split, the bhsd transpose and
        RoPE. With cp_group set, S is the LOCAL sequence shard and
        attention runs the xGMI ring."""
        if cache is None:
            cache = no_cache if cp_group is None else _NoCache(cp_group)
        return self._block(res, pending, K.rope_qkv, cos_t, sin_t, cache,
                           layer_idx)

    def decode_step(self, res, pending, c_rows, s_rows, view, layer_idx):
        """Continuous-batching decode: one new token per slot, each at
        its OWN cache position; ``view`` is the cache's decode_view of
        this step (models/kv_cache.py)."""
        return self._block(res, pending, self._rope_qkv_rows, c_rows,
                           s_rows, view, layer_idx)


class LlamaForCausalLM(nn.Module):
    """Set ``cp_group`` (a torch.distributed group) for context-parallel
    training: every rank in the group holds the SAME parameters but a
    different contiguous sequence shard of each batch (rank r gets token
    rows r*Sc..(r+1)*Sc); attention runs over the xGMI ring. Parameters
    being replicated, the per-rank local-mean losses backprop to grads
    whose cp-group AVERAGE is the true global-mean-loss gradient — i.e.
    cp ranks join the flat-buffer DDP all-reduce exactly like extra data-
    parallel ranks (parallel/ddp.py needs no changes)."""

    #: decode_step is free of data-dependent shapes -> the serving
    #: engine may capture it in a hipGraph and replay per token
    graph_safe_decode = True

    def __init__(self, cfg: LlamaConfig, cp_group=None):
        super().__init__()
        self.cfg = cfg
        self.cp_group = cp_group
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden_size,
                                  dtype=torch.bfloat16)
        self.layers = nn.ModuleList(
            DecoderLayer(cfg) for _ in range(cfg.num_layers))
        self.final_norm = RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.lm_head = Linear(cfg.hidden_size, cfg.vocab_size)
        cos_t, sin_t = K.rope_tables(cfg.max_seq_len, cfg.head_dim,
                                     cfg.rope_theta)
        self.register_buffer("cos_t", cos_t, persistent=False)
        self.register_buffer("sin_t", sin_t, persistent=False)
        self.reset_parameters()

    def reset_parameters(self):
        std = 0.02
        for name, p in self.named_parameters():
            if p.dim() >= 2:
                nn.init.normal_(p, mean=0.0, std=std)
            elif "norm" in name:
                nn.init.ones_(p)
        # scaled init for output projections (GPT-2 style)
        scale = 1.0 / math.sqrt(2 * self.cfg.num_layers)
        for layer in self.layers:
            layer.o_proj.weight.data.mul_(scale)
            layer.down_proj.weight.data.mul_(scale)

    PROJECTIONS = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj")

    @torch.no_grad()
    def quantize_weights_(self, lm_head=True):
        """Weight-only FP8 for serving: replace the four projections of
        every layer, and ``lm_head`` on request, by Fp8WeightLinear (E4M3
        bytes and one scale per output row) and free the bf16 parameters.
        The decode step then streams half the bytes. Every weight must be a
        multiple of 128 both ways (gate|up: per half); training through
        quantised projections is not supported. Returns self."""
        if self.cfg.fp8:
            raise ValueError(
                "quantize_weights_ is weight-only FP8 for serving; cfg.fp8 "
                "is the training format (ops/fp8.py) and does not combine "
                "with it")
        todo = [("layers.%d.%s" % (i, n), layer, n)
                for i, layer in enumerate(self.layers)
                for n in self.PROJECTIONS]
        if lm_head:
            todo.append(("lm_head", self, "lm_head"))
        todo = [t for t in todo
                if not isinstance(getattr(t[1], t[2]), Fp8WeightLinear)]
        for name, owner, attr in todo:
            dout, din = getattr(owner, attr).weight.shape
            halves = 2 if attr == "gate_up_proj" else 1
            if din % 128 or dout % (128 * halves):
                raise ValueError(
                    "quantize_weights_: %s is [%d, %d]; the FP8 stream "
                    "kernel needs multiples of 128 (per half of gate|up)"
                    % (name, dout, din))
        for _, owner, attr in todo:
            setattr(owner, attr,
                    Fp8WeightLinear.from_linear(getattr(owner, attr)))
        return self

    def forward(self, tokens, targets=None, cache=None):
        """tokens [B, S] int64 (the LOCAL shard when cp_group is set);
        returns mean loss over the local tokens if targets given, else
        logits. With ``cache`` (a KVCache, or a PagedSlotView of one
        slot of a PagedKVCache), S may be a suffix of an ongoing
        sequence starting at position cache.pos."""
        S = tokens.size(1)
        off = cache.pos if cache is not None else 0
        if self.cp_group is not None:
            import torch.distributed as dist

            off = dist.get_rank(self.cp_group) * S
        cos_t = self.cos_t[off:off + S].contiguous() if off else self.cos_t
        sin_t = self.sin_t[off:off + S].contiguous() if off else self.sin_t
        res = self.embed(tokens)
        pending = None
        recompute = (self.cfg.recompute and torch.is_grad_enabled()
                     and cache is None)
        for li, layer in enumerate(self.layers):
            if recompute:
                from torch.utils.checkpoint import checkpoint

                res, pending = checkpoint(
                    layer, res, pending, cos_t, sin_t, self.cp_group,
                    cache, li, use_reentrant=False)
            else:
                res, pending = layer(res, pending, cos_t, sin_t,
                                     self.cp_group, cache, li)
        if cache is not None:
            cache.pos += S
        _, x = K.add_rmsnorm(res, pending, self.final_norm.weight,
                             self.final_norm.eps)
        if targets is None:
            return self.lm_head(x)
        logits = self.lm_head(x)
        B, S, V = logits.shape
        loss = K.cross_entropy(logits.reshape(B * S, V),
                               targets.reshape(B * S))
        return loss.mean()

    @torch.no_grad()
    def decode_step(self, tokens, cache, positions, max_len=None):
        """One batched decode step for continuous batching: tokens
        [B, 1], positions[b] = this token's cache position for slot b
        (slots may sit at DIFFERENT positions; inactive slots pass 0 and
        their output row is garbage the batcher discards). ``cache`` is
        a KVCache or a PagedKVCache; on the paged cache a position of -1
        marks a slot that takes no part (nothing written, length 0).
        Returns logits [B, 1, V].

        With ``max_len`` (the cache capacity) the whole step is free of
        host reads and is hipGraph-capturable: the serving engine
        captures it once and replays per token (decode is launch-bound;
        see serving.ContinuousBatcher(graph=True))."""
        view = cache.decode_view(positions, tokens.device, max_len)
        c_rows = self.cos_t[view.rope_rows]
        s_rows = self.sin_t[view.rope_rows]
        res = self.embed(tokens)
        pending = None
        for li, layer in enumerate(self.layers):
            res, pending = layer.decode_step(res, pending, c_rows,
                                             s_rows, view, li)
        _, x = K.add_rmsnorm(res, pending, self.final_norm.weight,
                             self.final_norm.eps)
        return self.lm_head(x)

    def generate(self, tokens, max_new_tokens, temperature=0.0,
                 top_k=None, top_p=None, seed=None):
        return generate(self, tokens, max_new_tokens, temperature, top_k,
                        top_p, seed)

    def num_params(self):
        return sum(p.numel() for p in self.parameters())
