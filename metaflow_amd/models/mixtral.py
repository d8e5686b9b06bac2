"""Mixtral-style MoE on the metaflow_amd kernel library.

BASELINE config 5: Mixtral 8x7B @parallel train step with expert
all-to-all. Expert parallelism over RCCL/xGMI: experts are sharded across
ranks; tokens are routed top-k, exchanged with all_to_all_single (variable
splits, autograd-wrapped so backward is the transposed all-to-all), run
through the owner's experts (ops.swiglu + hipBLASLt GEMMs), exchanged back
and combined with routing weights. xGMI note: all-to-all is
point-to-point and uses all 7 links concurrently — better suited to the
topology than ring collectives.
"""

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import kernels as K
from .generate import generate
from .llama import Linear, RMSNorm, no_cache, rope_rows


@dataclass
class MixtralConfig:
    vocab_size: int = 32000
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    num_experts: int = 8
    top_k: int = 2
    max_seq_len: int = 8192
    rope_theta: float = 1000000.0
    rms_eps: float = 1e-5
    # decode_step runs the MoE block through the fused device-routed
    # kernels (ops/csrc/moe.hip): no host read, hipGraph-capturable
    fused_moe_decode: bool = False
    # forward (prefill, verify blocks, generate's prompt pass) runs the MoE
    # block through the same fused call when no grad is required and there
    # is no expert parallelism; large batches take the tiled kernels of
    # ops/csrc/moe_prefill.hip
    fused_moe_prefill: bool = False

    @classmethod
    def mixtral_8x7b(cls):
        return cls()

    @classmethod
    def mixtral_2x7b(cls):
        """Same per-layer/per-expert geometry as 8x7b but 2 experts
        (top-1): ~13.5B params — the largest Mixtral shape whose
        12 B/param training state (bf16 p+g, fp32 m+v) fits ONE
        MI355X's 288 GB, so the MoE hot path (router, grouped expert
        GEMMs, token scatter/gather) is MEASURABLE on a 1-GPU box.
        Honest label: this is NOT config 5's 8x7b — the full model needs
        the 8-GPU expert-parallel run (ep_group all-to-all path)."""
        return cls(num_experts=2, top_k=1)

    @classmethod
    def tiny(cls, vocab=1024, seq=256):
        return cls(vocab_size=vocab, hidden_size=256, intermediate_size=512,
                   num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128,
                   num_experts=4, top_k=2, max_seq_len=seq)


def _a2a_single(out, inp, out_splits, in_splits, group):
    """all_to_all_single, with a send/recv emulation for gloo (which has no
    all-to-all) so the EP path is CPU-testable with world_size > 1."""
    import torch.distributed as dist

    if dist.get_backend(group) != "gloo":
        dist.all_to_all_single(out, inp, output_split_sizes=out_splits,
                               input_split_sizes=in_splits, group=group)
        return
    rank = dist.get_rank(group)
    world = dist.get_world_size(group)
    in_off = [0]
    for s in in_splits:
        in_off.append(in_off[-1] + s)
    out_off = [0]
    for s in out_splits:
        out_off.append(out_off[-1] + s)
    # local copy + pairwise exchanges
    out[out_off[rank]:out_off[rank + 1]] = inp[in_off[rank]:
                                               in_off[rank + 1]]
    reqs = []
    for peer in range(world):
        if peer == rank:
            continue
        send = inp[in_off[peer]:in_off[peer + 1]].contiguous()
        reqs.append(dist.isend(send, peer, group=group))
    for peer in range(world):
        if peer == rank:
            continue
        recv = out.new_empty((out_splits[peer],) + tuple(out.shape[1:]))
        dist.recv(recv, peer, group=group)
        out[out_off[peer]:out_off[peer + 1]] = recv
    for r in reqs:
        r.wait()


class _AllToAll(torch.autograd.Function):
    """all_to_all_single with explicit splits; backward = transposed."""

    @staticmethod
    def forward(ctx, x, out_splits, in_splits, group):
        ctx.splits = (out_splits, in_splits)
        ctx.group = group
        out = x.new_empty((sum(out_splits),) + tuple(x.shape[1:]))
        _a2a_single(out, x.contiguous(), out_splits, in_splits, group)
        return out

    @staticmethod
    def backward(ctx, grad):
        out_splits, in_splits = ctx.splits
        gin = grad.new_empty((sum(in_splits),) + tuple(grad.shape[1:]))
        _a2a_single(gin, grad.contiguous(), in_splits, out_splits,
                    ctx.group)
        return gin, None, None, None


def all_to_all(x, out_splits, in_splits, group=None):
    return _AllToAll.apply(x, out_splits, in_splits, group)


class Expert(nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.gate_proj = Linear(hidden, inter)
        self.up_proj = Linear(hidden, inter)
        self.down_proj = Linear(inter, hidden)

    def forward(self, x):
        return self.down_proj(K.swiglu(self.gate_proj(x), self.up_proj(x)))


class Fp8Expert(nn.Module):
    """An Expert with weight-only FP8 weights: E4M3 bytes and one fp32
    scale per output row (K.moe_quant_weight), held as buffers, so
    state_dict round-trips and there is nothing to train. The fused MoE
    block reads bytes and scales as they are (K.MoeTable with scales);
    ``forward`` is the eager fallback for the CPU, expert parallelism and
    batches above the fused thresholds: dequantise to bf16, then Expert's
    GEMMs and K.swiglu. It is differentiable in x."""

    NAMES = ("gate_proj", "up_proj", "down_proj")

    def __init__(self, hidden, inter, device=None):
        super().__init__()
        for name, (dout, din) in zip(self.NAMES, ((inter, hidden),
                                                  (inter, hidden),
                                                  (hidden, inter))):
            self.register_buffer(name + "_w8", torch.zeros(
                dout, din, dtype=torch.float8_e4m3fn, device=device))
            self.register_buffer(name + "_scale", torch.ones(
                dout, dtype=torch.float32, device=device))

    @classmethod
    def from_expert(cls, expert):
        w = expert.gate_proj.weight
        q = cls(w.size(1), w.size(0), device=w.device)
        for name in cls.NAMES:
            w8, scale = K.moe_quant_weight(getattr(expert, name).weight)
            getattr(q, name + "_w8").copy_(w8)
            getattr(q, name + "_scale").copy_(scale)
        return q

    def weight(self, name, dtype=torch.bfloat16):
        return K.moe_dequant_ref(getattr(self, name + "_w8"),
                                 getattr(self, name + "_scale"), dtype)

    def forward(self, x):
        from ..ops.gemm import tuned_linear

        g = tuned_linear(x, self.weight("gate_proj", x.dtype))
        u = tuned_linear(x, self.weight("up_proj", x.dtype))
        return tuned_linear(K.swiglu(g, u), self.weight("down_proj", x.dtype))


class MoELayer(nn.Module):
    """Top-k router + (optionally expert-parallel) experts.

    With EP (world > 1): rank r owns experts [r*E/W, (r+1)*E/W); the
    dispatch is a single all-to-all of the routed token copies, grouped by
    destination rank.
    """

    def __init__(self, cfg: MixtralConfig, ep_group=None):
        super().__init__()
        self.cfg = cfg
        self.router = Linear(cfg.hidden_size, cfg.num_experts)
        self.ep_group = ep_group
        import torch.distributed as dist

        if (dist.is_available() and dist.is_initialized()
                and dist.get_world_size(ep_group) > 1
                and cfg.num_experts % dist.get_world_size(ep_group) == 0):
            self.ep_world = dist.get_world_size(ep_group)
            self.ep_rank = dist.get_rank(ep_group)
        else:
            self.ep_world = 1
            self.ep_rank = 0
        self.experts_per_rank = cfg.num_experts // self.ep_world
        self.local_experts = nn.ModuleList(
            Expert(cfg.hidden_size, cfg.intermediate_size)
            for _ in range(self.experts_per_rank))
        if self.ep_world > 1:
            # grads are complete after the token all-to-all: exclude from
            # the DP all-reduce (see FlatParamModel no-sync region)
            for p in self.local_experts.parameters():
                p._mfx_no_sync = True

    # forward's fused block, chosen from shapes by the mean expert run
    # T * top_k / E. Up to TILED_MEAN_RUN entries the stream kernels: they
    # serve an expert in groups of 32 entries and read its weights again
    # for every further group, and at 8x7B geometry they win up to a mean
    # run of 28 and lose from 30 on, where some expert passes 32. Above
    # that the tiled kernels, up to TILED_MAX_MEAN_RUN: measured faster
    # than the eager block up to a mean run of 384 and slower from 512 on
    # (docs/KERNELS.md, "MoE prefill"), so larger batches stay eager.
    TILED_MEAN_RUN = 28
    TILED_MAX_MEAN_RUN = 384
    # Quantised experts (docs/KERNELS.md, "FP8 expert weights"): the E4M3
    # stream reads half the bytes per group and the tiled kernels, bound by
    # LDS, gain nothing from them, so the stream wins up to a mean run of 48
    # (every run, also past the second group) and loses from 64 on. The
    # eager block here is the dequantising fallback, which rewrites every
    # expert in bf16 per call: the tiled kernels won at every size
    # measured, up to a mean run of 1024.
    TILED_MEAN_RUN_FP8 = 48
    TILED_MAX_MEAN_RUN_FP8 = 1024

    def _fused_path(self, T):
        """"stream", "tiled" or None (the eager block) for T tokens."""
        run = T * self.cfg.top_k
        E = self.cfg.num_experts
        q = self.quantized
        if run <= (self.TILED_MEAN_RUN_FP8 if q
                   else self.TILED_MEAN_RUN) * E and \
                run <= K.MOE_STREAM_MAX_ENTRIES:
            return "stream"
        if run <= (self.TILED_MAX_MEAN_RUN_FP8 if q
                   else self.TILED_MAX_MEAN_RUN) * E and \
                run <= K.MOE_MAX_ENTRIES:
            return "tiled"
        return None

    @property
    def quantized(self):
        return len(self.local_experts) > 0 and all(
            isinstance(e, Fp8Expert) for e in self.local_experts)

    @torch.no_grad()
    def quantize_experts_(self):
        """Replace every Expert by an Fp8Expert of its weights (E4M3 bytes,
        one scale per output row) and free the bf16 parameters. The fused
        block then streams half the bytes; training through quantised
        experts is not supported (they have no parameters)."""
        for i, e in enumerate(self.local_experts):
            if not isinstance(e, Fp8Expert):
                self.local_experts[i] = Fp8Expert.from_expert(e)
        self._moe_table = None
        return self

    def _table(self):
        """The cached K.MoeTable of the local experts, rebuilt when a
        weight or scale has moved (a host-side comparison of
        data_ptr()s)."""
        ex = self.local_experts
        if self.quantized:
            ws = [[getattr(e, n + "_w8") for e in ex]
                  for n in Fp8Expert.NAMES]
            scales = [[getattr(e, n + "_scale") for e in ex]
                      for n in Fp8Expert.NAMES]
        else:
            ws = [[getattr(e, n).weight for e in ex]
                  for n in Fp8Expert.NAMES]
            scales = None
        table = getattr(self, "_moe_table", None)
        if table is None or \
                table.ptrs != K.MoeTable.addresses(*ws, scales=scales):
            table = self._moe_table = K.MoeTable(*ws, scales=scales)
        return table

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad
                                   for p in self.parameters()))

    def forward(self, x):
        cfg = self.cfg
        if (cfg.fused_moe_prefill and self.ep_world == 1
                and not self._wants_grad(x)):
            path = self._fused_path(x.numel() // x.size(-1))
            if path is not None:
                return self.decode(x, path)
        B, S, h = x.shape
        flat = x.reshape(B * S, h)
        logits = self.router(flat).float()
        # softmax over all experts, top-k, renormalise: the same weights as
        # the fused block's softmax over the selected logits, since the
        # normaliser of the full softmax cancels in the renormalisation
        probs = torch.softmax(logits, dim=-1)
        weights, experts = probs.topk(cfg.top_k, dim=-1)  # [N, k]
        weights = weights / weights.sum(-1, keepdim=True)

        N = flat.size(0)
        k = cfg.top_k
        # one entry per (token, choice): sort by destination expert
        flat_expert = experts.reshape(-1)              # [N*k]
        order = torch.argsort(flat_expert, stable=True)
        token_idx = order // k                         # source token
        sorted_expert = flat_expert[order]
        counts = torch.bincount(sorted_expert, minlength=cfg.num_experts)

        dispatched = flat[token_idx]                   # [N*k, h]

        if self.ep_world > 1:
            import torch.distributed as dist

            # counts per destination rank
            per_rank = counts.reshape(self.ep_world,
                                      self.experts_per_rank).sum(-1)
            in_splits = per_rank.tolist()
            recv_counts = torch.empty(
                self.ep_world * self.experts_per_rank, dtype=counts.dtype,
                device=counts.device)
            # exchange per-expert counts so the owner can group its input
            _a2a_single(recv_counts, counts.contiguous(),
                        [self.experts_per_rank] * self.ep_world,
                        [self.experts_per_rank] * self.ep_world,
                        self.ep_group)
            out_splits = recv_counts.reshape(
                self.ep_world, self.experts_per_rank).sum(-1).tolist()
            incoming = all_to_all(dispatched, out_splits, in_splits,
                                  self.ep_group)
            # incoming is grouped by (source rank, local expert); regroup
            # by local expert
            blocks = []
            offsets = []
            off = 0
            rc = recv_counts.reshape(self.ep_world, self.experts_per_rank)
            for sr in range(self.ep_world):
                for le in range(self.experts_per_rank):
                    n = int(rc[sr, le])
                    offsets.append((le, off, n))
                    off += n
            outs = incoming.new_empty(incoming.shape)
            for le in range(self.experts_per_rank):
                segs = [incoming[o:o + n] for (l, o, n) in offsets
                        if l == le and n > 0]
                if segs:
                    y = self.local_experts[le](torch.cat(segs))
                    # scatter back into position
                    pos = 0
                    for (l, o, n) in offsets:
                        if l == le and n > 0:
                            outs[o:o + n] = y[pos:pos + n]
                            pos += n
            returned = all_to_all(outs, in_splits, out_splits,
                                  self.ep_group)
        else:
            returned = dispatched.new_empty(dispatched.shape)
            off = 0
            for e in range(cfg.num_experts):
                n = int(counts[e])
                if n > 0:
                    returned[off:off + n] = self.local_experts[e](
                        dispatched[off:off + n])
                off += n

        # combine: weight each routed copy and scatter-add to source token
        w_sorted = weights.reshape(-1)[order].to(returned.dtype)
        contrib = returned * w_sorted.unsqueeze(-1)
        out = torch.zeros_like(flat)
        out.index_add_(0, token_idx, contrib)
        return out.reshape(B, S, h)

    def decode(self, x, path="stream"):
        """The fused block, inference-only and without EP: the router
        GEMM, then K.moe_ffn (device routing, grouped expert kernels) on
        ``path``: the stream kernels at decode, and from forward with
        cfg.fused_moe_prefill whichever the batch size calls for. Reads
        nothing back, unlike forward's per-expert counts. The table of
        weight addresses is cached and rebuilt when a weight has moved (a
        host-side comparison of data_ptr()s); after quantize_experts_ it
        is the E4M3 table and the call takes the E4M3 kernels."""
        assert self.ep_world == 1, "fused MoE decode has no EP path"
        B, S, h = x.shape
        flat = x.reshape(B * S, h)
        logits = self.router(flat).float()
        table = self._table()
        if flat.size(0) * self.cfg.top_k > K.MOE_STREAM_MAX_ENTRIES:
            path = "tiled"
        out = K.moe_ffn(flat, logits, table, top_k=self.cfg.top_k,
                        path=path)
        return out.reshape(B, S, h)


class MixtralDecoderLayer(nn.Module):
    def __init__(self, cfg: MixtralConfig, ep_group=None):
        super().__init__()
        self.cfg = cfg
        h, hd = cfg.hidden_size, cfg.head_dim
        self.input_norm = RMSNorm(h, cfg.rms_eps)
        self.q_proj = Linear(h, cfg.num_heads * hd)
        self.k_proj = Linear(h, cfg.num_kv_heads * hd)
        self.v_proj = Linear(h, cfg.num_kv_heads * hd)
        self.o_proj = Linear(cfg.num_heads * hd, h)
        self.post_norm = RMSNorm(h, cfg.rms_eps)
        self.moe = MoELayer(cfg, ep_group)

    def _block(self, x, heads, cos, sin, view, layer_idx, moe=None):
        """The layer body. ``heads(y, cos, sin)`` projects the normed
        input to the roped q, k, v in [B,H,S,D]; ``view`` attends; ``moe``
        is the MoE block's entry (its forward unless given)."""
        cfg = self.cfg
        B, S, _ = x.shape
        q, k, v = heads(self.input_norm(x), cos, sin)
        o = view.attend(layer_idx, q, k, v, S, 1.0 / math.sqrt(cfg.head_dim))
        o = o.transpose(1, 2).reshape(B, S, cfg.num_heads * cfg.head_dim)
        x = x + self.o_proj(o)
        return x + (moe or self.moe)(self.post_norm(x))

    def _seq_heads(self, y, cos_t, sin_t):
        cfg = self.cfg
        B, S, _ = y.shape
        hd = cfg.head_dim
        q = K.rope(self.q_proj(y).view(B, S, cfg.num_heads, hd),
                   cos_t, sin_t).transpose(1, 2)
        k = K.rope(self.k_proj(y).view(B, S, cfg.num_kv_heads, hd),
                   cos_t, sin_t).transpose(1, 2)
        v = self.v_proj(y).view(B, S, cfg.num_kv_heads, hd)
        return q, k, v.transpose(1, 2)

    def _row_heads(self, y, c_rows, s_rows):
        B, hd = y.size(0), self.cfg.head_dim
        q = self.q_proj(y).view(B, 1, -1, hd).transpose(1, 2)
        k = self.k_proj(y).view(B, 1, -1, hd).transpose(1, 2)
        v = self.v_proj(y).view(B, 1, -1, hd).transpose(1, 2)
        return rope_rows(q, c_rows, s_rows), rope_rows(k, c_rows, s_rows), v

    def forward(self, x, cos_t, sin_t, cache=None, layer_idx=0):
        return self._block(x, self._seq_heads, cos_t, sin_t,
                           no_cache if cache is None else cache, layer_idx)

    def decode_step(self, x, c_rows, s_rows, view, layer_idx):
        """Continuous-batching decode for the MoE layer: ``view`` is the
        cache's decode_view of this step; experts route per decoded
        token. With cfg.fused_moe_decode (and no expert parallelism) the
        MoE block runs MoELayer.decode."""
        fused = self.cfg.fused_moe_decode and self.moe.ep_world == 1
        return self._block(x, self._row_heads, c_rows, s_rows, view,
                           layer_idx, self.moe.decode if fused else None)


class MixtralForCausalLM(nn.Module):
    def __init__(self, cfg: MixtralConfig, ep_group=None):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden_size,
                                  dtype=torch.bfloat16)
        self.layers = nn.ModuleList(
            MixtralDecoderLayer(cfg, ep_group)
            for _ in range(cfg.num_layers))
        self.final_norm = RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.lm_head = Linear(cfg.hidden_size, cfg.vocab_size)
        cos_t, sin_t = K.rope_tables(cfg.max_seq_len, cfg.head_dim,
                                     cfg.rope_theta)
        self.register_buffer("cos_t", cos_t, persistent=False)
        self.register_buffer("sin_t", sin_t, persistent=False)
        self.reset_parameters()

    @property
    def graph_safe_decode(self):
        """decode_step reads nothing back from the device exactly when
        every layer's MoE block takes the fused path."""
        return self.cfg.fused_moe_decode and all(
            layer.moe.ep_world == 1 for layer in self.layers)

    def reset_parameters(self):
        for p in self.parameters():
            if p.dim() >= 2:
                nn.init.normal_(p, mean=0.0, std=0.02)

    def quantize_experts_(self):
        """Weight-only FP8 for every layer's experts
        (MoELayer.quantize_experts_); attention, router and lm_head stay
        bf16. Inference-only from here on."""
        for layer in self.layers:
            layer.moe.quantize_experts_()
        return self

    def forward(self, tokens, targets=None, cache=None):
        S = tokens.size(1)
        off = cache.pos if cache is not None else 0
        cos_t = self.cos_t[off:off + S].contiguous() if off else self.cos_t
        sin_t = self.sin_t[off:off + S].contiguous() if off else self.sin_t
        x = self.embed(tokens)
        for li, layer in enumerate(self.layers):
            x = layer(x, cos_t, sin_t, cache, li)
        if cache is not None:
            cache.pos += S
        x = self.final_norm(x)
        logits = self.lm_head(x)
        if targets is None:
            return logits
        B, S, V = logits.shape
        loss = K.cross_entropy(logits.reshape(B * S, V),
                               targets.reshape(B * S))
        return loss.mean()

    @torch.no_grad()
    def decode_step(self, tokens, cache, positions, max_len=None):
        """One batched decode step for continuous batching (same
        contract as LlamaForCausalLM.decode_step: per-slot cache
        positions, varlen flash-decode). With the eager MoE block it is
        NOT hipGraph-capturable — the router's token dispatch is
        shape-dynamic and read on the host — so the serving engine keeps
        Mixtral on the eager decode path; with cfg.fused_moe_decode it
        is (graph_safe_decode)."""
        view = cache.decode_view(positions, tokens.device, max_len)
        c_rows = self.cos_t[view.rope_rows]
        s_rows = self.sin_t[view.rope_rows]
        x = self.embed(tokens)
        for li, layer in enumerate(self.layers):
            x = layer.decode_step(x, c_rows, s_rows, view, li)
        return self.lm_head(self.final_norm(x))

    def generate(self, tokens, max_new_tokens, temperature=0.0,
                 top_k=None, top_p=None, seed=None):
        return generate(self, tokens, max_new_tokens, temperature, top_k,
                        top_p, seed)

    def num_params(self):
        return sum(p.numel() for p in self.parameters())
