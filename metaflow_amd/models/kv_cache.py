"""KV caches of the in-house model family, and which attention kernel
each cached call runs.

Two cache kinds, one interface with three parts:

* sequence mode (the models' ``forward(tokens, cache=...)``): the object
  holds one running ``pos``; ``attend`` writes the S new K/V rows there
  and attends. A KVCache is used whole (generate, speculation) or
  through ``slot_view(slot)`` (the serving engine's prefill); a
  PagedKVCache only through its slot views.
* batch mode (``decode_step``): ``decode_positions`` + ``decode_attend``,
  one new row per slot, each slot at its own position.
* engine hooks (serving.ContinuousBatcher): ``admit``, ``ensure``,
  ``sync``, ``release``, ``idle_position``.

Kernels are always reached as attributes of ops.kernels (``K.name``).
"""

import torch

from ..ops import kernels as K


class _DenseRows(object):
    """Sequence mode over dense rows: k/v hold one [B, Hkv, max_len, 128]
    tensor per layer, ``pos`` is the number of cached positions (advanced
    once per model forward, not per layer)."""

    def __init__(self, k, v):
        self.k = k
        self.v = v
        self.pos = 0

    def attend(self, layer_idx, q, k, v, S, scale):
        """Write the S new K/V rows at ``pos``, then attend. S is q's row
        count, which the caller has at hand: reading it off the tensor
        here costs more than the call itself, once per layer on a
        launch-bound decode step."""
        kc, vc, pos = self.k[layer_idx], self.v[layer_idx], self.pos
        kc[:, :, pos:pos + S] = k
        vc[:, :, pos:pos + S] = v
        if pos == 0:
            # prefill: flash (padded to the 256 tile internally for
            # unaligned prompts)
            return K.attention(q, k, v)
        if S == 1:
            # one-token decode: split-K flash-decode straight over the
            # cache allocation (decode.hip)
            return K.attn_decode(q, kc, vc, pos + 1, scale)
        # S new rows at pos > 0 (speculative verify block, later prefill
        # chunks): append kernel over the whole cache allocation
        # (append.hip)
        return K.attn_append(q, kc, vc, pos, scale)


class KVCache(_DenseRows):
    """Preallocated per-layer KV cache for autoregressive decode, filled
    in place as positions arrive: max_len rows reserved per sequence."""

    def __init__(self, cfg, batch, max_len, device, dtype=torch.bfloat16):
        k = [torch.zeros(batch, cfg.num_kv_heads, max_len, cfg.head_dim,
                         device=device, dtype=dtype)
             for _ in range(cfg.num_layers)]
        super().__init__(k, [torch.zeros_like(t) for t in k])
        self.max_len = max_len

    def slot_view(self, slot):
        """Single-slot view with its own ``pos``: a prefill writes
        through it in place (views, no copies)."""
        return _DenseRows([t[slot:slot + 1] for t in self.k],
                          [t[slot:slot + 1] for t in self.v])

    def decode_positions(self, positions, device):
        """Device tensors of one batched decode step: (pos_t, lengths,
        rope_rows). Every slot writes at positions[b]. No host read."""
        pos_t = torch.as_tensor(positions, device=device, dtype=torch.long)
        return pos_t, (pos_t + 1).to(torch.int32), pos_t

    def decode_attend(self, layer_idx, q, k, v, pos_t, lengths, scale,
                      max_len=None):
        """One layer of the batched decode step: per-slot scatter of the
        new row, then the varlen flash-decode over the full allocation."""
        kc, vc = self.k[layer_idx], self.v[layer_idx]
        bidx = torch.arange(q.size(0), device=q.device)
        kc[bidx, :, pos_t] = k[:, :, 0]
        vc[bidx, :, pos_t] = v[:, :, 0]
        return K.attn_decode_varlen(q.contiguous(), kc, vc, lengths, scale,
                                    max_len=max_len)

    # engine hooks: every slot owns its max_len rows from the start
    def admit(self, slot, n_rows):
        return True

    def ensure(self, slot, n_rows):
        pass

    def sync(self):
        pass

    def release(self, slot):
        pass

    def idle_position(self, rows_cached):
        """The batched decode scatters a (garbage) K/V row for EVERY
        slot; one that is not decoding aims it at its next-unwritten row
        — the following prefill chunk overwrites it, so the cached prefix
        stays intact."""
        return rows_cached


class PagedKVCache(object):
    """Paged KV cache for the serving engine: instead of max_len rows per
    slot, sequences own 64-row pages of a shared pool and a block table
    maps (slot, page index) -> pool page (ops/csrc/paged.hip).

    k_pages/v_pages: one [num_pages, Hkv, 64, 128] tensor per layer (all
    layers share one table: a page index means the same page in each).
    ``table_host`` is the int32 [max_batch, ceil(max_len/64)] host mirror
    the allocator edits; ``block_table`` is the persistent device copy the
    kernels read, refreshed by ``sync()``. -1 = no page.

    The free list is LIFO. Reservations only count pages (admission
    control); pages are handed out by ``ensure``. Freed pages are not
    cleared: rows past a sequence's length are never read.
    """

    PAGE = K.PAGE_ROWS

    def __init__(self, cfg, num_pages, max_batch, max_len, device,
                 dtype=torch.bfloat16):
        self.k_pages = [torch.zeros(num_pages, cfg.num_kv_heads, self.PAGE,
                                    cfg.head_dim, device=device,
                                    dtype=dtype)
                        for _ in range(cfg.num_layers)]
        self.v_pages = [torch.zeros_like(k) for k in self.k_pages]
        self.num_pages = num_pages
        self.max_batch = max_batch
        self.max_len = max_len
        self.pages_per_seq = -(-max_len // self.PAGE)
        self.table_host = torch.full((max_batch, self.pages_per_seq), -1,
                                     dtype=torch.int32)
        # its own storage even on the CPU: the mirror is edited freely,
        # the kernels' table changes only in sync()
        self.block_table = torch.full_like(self.table_host, -1,
                                           device=device)
        self._free = list(range(num_pages - 1, -1, -1))  # pop() -> page 0
        self._owned = [[] for _ in range(max_batch)]
        self._reserved = 0
        self._admitted = [0] * max_batch  # pages reserved by admit()
        self._dirty = False

    @property
    def free_pages(self):
        return len(self._free)

    def reserve(self, n_pages):
        """Count n_pages against the pool; False if they do not fit."""
        if self._reserved + n_pages > self.num_pages:
            return False
        self._reserved += n_pages
        return True

    def release_reservation(self, n_pages):
        assert 0 <= n_pages <= self._reserved, "released more than reserved"
        self._reserved -= n_pages

    def ensure(self, slot, n_rows):
        """Allocate pages until ``slot`` covers rows 0 .. n_rows-1."""
        need = -(-n_rows // self.PAGE)
        assert need <= self.pages_per_seq, "rows beyond the slot capacity"
        owned = self._owned[slot]
        while len(owned) < need:
            assert self.num_pages - len(self._free) < self._reserved, \
                "page allocation beyond the reservation"
            page = self._free.pop()
            self.table_host[slot, len(owned)] = page
            owned.append(page)
            self._dirty = True

    def free_slot(self, slot):
        """Return the slot's pages to the pool, reset its entries."""
        owned = self._owned[slot]
        assert owned, "double free: slot %d owns no pages" % slot
        self._free.extend(reversed(owned))
        self.table_host[slot, :len(owned)] = -1
        self._owned[slot] = []
        self._dirty = True

    def sync(self):
        """One copy of the host table into the device table, only when
        the host table changed since the last sync."""
        if self._dirty:
            self.block_table.copy_(self.table_host)
            self._dirty = False

    def slot_view(self, slot):
        return PagedSlotView(self, slot)

    def decode_positions(self, positions, device):
        """Device tensors of one batched decode step: (pos_t, lengths,
        rope_rows). A position of -1 marks a slot that does not take
        part: pos_t (int32, the write offsets) keeps the -1 so the write
        skips it, its length is 0 and its RoPE row is clamped to 0. No
        host read."""
        pos_t = torch.as_tensor(positions, device=device, dtype=torch.long)
        return (pos_t.to(torch.int32), (pos_t + 1).to(torch.int32),
                pos_t.clamp(min=0))

    def decode_attend(self, layer_idx, q, k, v, pos_t, lengths, scale,
                      max_len=None):
        """One layer of the batched decode step: one kv_page_write of
        every slot's new row, one paged flash-decode. The split count
        always comes from a capacity (max_len or the cache's), so eager
        and captured steps launch identical grids."""
        kp, vp = self.k_pages[layer_idx], self.v_pages[layer_idx]
        K.kv_page_write(k, v, kp, vp, self.block_table, pos_t)
        return K.attn_decode_paged(q.contiguous(), kp, vp, self.block_table,
                                   lengths, scale,
                                   self.max_len if max_len is None
                                   else max_len)

    # engine hooks
    def admit(self, slot, n_rows):
        """Reserve every page a request of n_rows total rows can ever
        touch, so it never runs out mid-decode; False (nothing reserved)
        if they do not fit now."""
        assert n_rows <= self.max_len, \
            "request longer than the slot capacity"
        need = -(-n_rows // self.PAGE)
        assert need <= self.num_pages, "request larger than the page pool"
        if not self.reserve(need):
            return False
        self._admitted[slot] = need
        return True

    def release(self, slot):
        self.free_slot(slot)
        self.release_reservation(self._admitted[slot])
        self._admitted[slot] = 0

    def idle_position(self, rows_cached):
        """No garbage-row trick here: a slot that is not decoding passes
        -1 (nothing written, length 0)."""
        return -1


class PagedSlotView(object):
    """Single-slot view of a PagedKVCache for the models' forward:
    prefill chunks of one request write through it and advance ``pos``."""

    def __init__(self, paged, slot):
        self.paged = paged
        self.slot = slot
        self.pos = 0

    def attend(self, layer_idx, q, k, v, S, scale):
        """Write the S new K/V rows at ``pos``, then attend. The first
        chunk (pos 0) is the flash prefill on the fresh tensors; a
        one-token step is the paged decode kernel; a later chunk is the
        paged append kernel, which reads the slot's pages in place
        through the block table (append.hip, paged instantiation)."""
        pc, slot, pos = self.paged, self.slot, self.pos
        assert q.size(0) == 1, "a paged slot view holds one sequence"
        kp, vp = pc.k_pages[layer_idx], pc.v_pages[layer_idx]
        table_row = pc.block_table[slot:slot + 1]
        K.kv_page_write(k, v, kp, vp, table_row, [pos])
        if pos == 0:
            return K.attention(q, k, v)
        if S == 1:
            return K.attn_decode_paged(q.contiguous(), kp, vp, table_row,
                                       [pos + 1], scale, pc.max_len)
        return K.attn_append_paged(q.contiguous(), kp, vp, table_row,
                                   [pos], scale)
