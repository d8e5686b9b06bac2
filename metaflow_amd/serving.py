"""Continuous-batching serving engine for the in-house model family.

Iteration-level scheduling (the vLLM/Orca idea, built MI355X-first on
our own kernels — no reference counterpart, SURVEY §2.4 note):

* a fixed pool of KV-cache SLOTS (one preallocated batched cache, full
  stride — the varlen flash-decode kernel reads each slot at its own
  valid length, decode.hip);
* new requests are admitted BETWEEN decode steps: the prompt prefills
  into a free slot through the flash fwd kernel (a [slot:slot+1] view
  of the batched cache — zero copies);
* every step decodes ONE token for all active slots in a single batched
  kernel pass (slots at different positions — per-slot RoPE rows +
  per-slot cache scatter, models/llama.py decode_step);
* finished slots free immediately and the queue refills them, so
  throughput tracks the arrival rate instead of the slowest member of a
  static batch;
* opt-in paging (``num_pages``): the slots share a pool of 64-row pages
  through a device block table instead of reserving max_len rows each
  (models/kv_cache.py PagedKVCache, paged.hip).

The engine never asks which cache it holds: admission, page allocation,
release and the position of a slot that is not decoding are hooks of
the cache (models/kv_cache.py).

Token selection is per request: ``temperature``, ``top_k``, ``top_p`` and
``seed`` ride on the Request (defaults: greedy). Every selection site is
one fused sampler launch over all rows (ops/kernels.py sample_tokens,
ops/csrc/sampling.hip) and ONE host read of the ids, outside the captured
decode graph. A request owns a CPU generator seeded with its seed; its
i-th token consumes the generator's i-th draw, wherever that token is
emitted, so a request's tokens depend neither on its batch neighbours,
nor on chunked or whole-prompt prefill, nor on eager or graph decode.

Greedy and sampled decoding are token-exact with ``model.generate`` per
request (``generate(prompt[None], n, temperature, top_k, top_p, seed)``).
"""

from collections import deque


class Request(object):
    _next_id = 0

    def __init__(self, prompt_tokens, max_new_tokens, temperature=0.0,
                 top_k=0, top_p=1.0, seed=None):
        self.id = Request._next_id
        Request._next_id += 1
        self.prompt = list(prompt_tokens)
        self.max_new = int(max_new_tokens)
        self.temperature = float(temperature or 0.0)
        self.top_k = int(top_k or 0)
        self.top_p = 1.0 if top_p is None else float(top_p)
        self.seed = seed
        # a greedy request draws nothing and leaves the default RNG alone
        self._gen = None
        if self.temperature > 0:
            from .models.generate import seeded_generator

            self._gen = seeded_generator(seed)
        self.generated = []
        self.done = False

    def draw(self):
        """The uniform that selects this request's next token."""
        if self._gen is None:
            return 0.0
        from .models.generate import draw

        return draw(self._gen)


class ContinuousBatcher(object):
    def __init__(self, model, max_batch=8, max_len=2048, graph="auto",
                 prefill_chunk=None, num_pages=None):
        """graph: capture the whole decode step in a hipGraph and replay
        it per token (decode is LAUNCH-bound — ~200 small kernels per
        step; replay collapses them to one submit). "auto" captures on
        GPU and falls back silently; the step stays host-read-free
        because the varlen kernel chunks from device lengths
        (decode.hip) and splits come from the cache capacity.

        prefill_chunk: bound per-step latency under long prompts — a
        newly admitted request prefills at most this many prompt tokens
        per step() instead of all at once, so active slots keep
        decoding every step instead of stalling behind a monolithic
        prefill (a slot mid-prefill sits at cache length
        positions[slot] and its decode row is masked by the varlen
        kernel's per-slot lengths). None = whole-prompt prefill at
        admission (lowest total latency when prompts are short).

        num_pages: None keeps the dense cache (max_len rows reserved per
        slot). An integer selects the paged cache instead: a pool of
        that many 64-row pages shared by all slots (models/kv_cache.py
        PagedKVCache, ops/csrc/paged.hip), so the number of concurrent
        requests is bounded by the rows they can actually reach, not by
        max_batch * max_len. Admission is FIFO and reserves
        ceil((len(prompt) + max_new) / 64) pages for the head request —
        it waits (and everything behind it) until they fit, so no
        request runs out of pages mid-decode and nothing is preempted.
        Physical pages are allocated lazily as rows are written."""
        import torch

        from .models.kv_cache import KVCache, PagedKVCache

        self.model = model
        self.max_batch = max_batch
        self.max_len = max_len
        device = next(model.parameters()).device
        self.device = device
        self.paged = num_pages is not None
        if self.paged:
            self.cache = PagedKVCache(model.cfg, num_pages, max_batch,
                                      max_len, device,
                                      dtype=model.embed.weight.dtype)
        else:
            self.cache = KVCache(model.cfg, max_batch, max_len, device,
                                 dtype=model.embed.weight.dtype)
        self.positions = [0] * max_batch    # cached tokens per slot
        self.slots = [None] * max_batch     # Request or None
        self.next_token = [0] * max_batch   # token to feed next step
        self.prefill_chunk = prefill_chunk
        self._views = [None] * max_batch    # slot view while prefilling
        self._prefill_done = [0] * max_batch  # prompt tokens cached
        self.queue = deque()
        self._torch = torch
        # per-slot sampling parameters as the sampler reads them; a slot
        # that is free or mid-prefill holds temperature 0 (its row of the
        # decode step is selected greedily and ignored)
        self._temp_host = [0.0] * max_batch
        self._topk_host = [0] * max_batch
        self._topp_host = [1.0] * max_batch
        self._params_stale = True
        self._graph = None
        if graph is True and not getattr(model, "graph_safe_decode",
                                         False):
            raise ValueError(
                "model's decode_step is not hipGraph-safe (data-"
                "dependent shapes, e.g. MoE routing)")
        if graph and device.type == "cuda" and \
                getattr(model, "graph_safe_decode", False):
            try:
                self._capture_graph()
            except Exception:
                if graph is True:
                    raise
                self._graph = None  # auto: eager decode

    def _capture_graph(self):
        torch = self._torch
        self._tok_buf = torch.zeros(self.max_batch, 1, dtype=torch.long,
                                    device=self.device)
        # no slot decodes while capturing
        self._pos_buf = torch.full((self.max_batch,),
                                   self.cache.idle_position(0),
                                   dtype=torch.long, device=self.device)
        # warmup on a side stream (allocator primes its graph pool)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.model.decode_step(self._tok_buf, self.cache,
                                       self._pos_buf,
                                       max_len=self.max_len)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._logits_buf = self.model.decode_step(
                self._tok_buf, self.cache, self._pos_buf,
                max_len=self.max_len)
        self._graph = g

    def _decode(self, tokens, positions):
        if self._graph is not None:
            torch = self._torch
            self._tok_buf.copy_(tokens)
            self._pos_buf.copy_(torch.as_tensor(positions,
                                                device=self.device))
            self._graph.replay()
            return self._logits_buf
        # no max_len: the dense cache sizes its splits from the lengths,
        # the paged cache from its capacity, as in the captured step
        return self.model.decode_step(tokens, self.cache, positions)

    def submit(self, prompt_tokens, max_new_tokens, temperature=0.0,
               top_k=0, top_p=1.0, seed=None):
        """Queue a request. Defaults decode greedily; temperature > 0
        samples with the optional top_k / top_p cuts, reproducibly for a
        given ``seed`` (None draws one from torch's default generator)."""
        req = Request(prompt_tokens, max_new_tokens, temperature, top_k,
                      top_p, seed)
        self.queue.append(req)
        return req

    # ------------------------------------------------------------ selection
    def _sample(self, rows, temperature, top_k, top_p, u_list):
        """One sampler launch over ``rows`` [R, V] and one host read:
        the R token ids as Python ints."""
        from .ops import kernels as K

        u = self._torch.tensor(u_list, dtype=self._torch.float32,
                               device=self.device)
        return K.sample_tokens(rows, temperature, top_k, top_p, u).tolist()

    def _first_token(self, slot, logits):
        """Emit a request's first token from its prefill logits
        [1, S, V] and hand the slot to the decode batch."""
        req = self.slots[slot]
        # the slot's parameters go live here: the first token reads its
        # one-row slice of the per-slot tensors, the decode steps the whole
        self._temp_host[slot] = req.temperature
        self._topk_host[slot] = req.top_k
        self._topp_host[slot] = req.top_p
        self._params_stale = True
        nxt = self._sample(
            logits[:, -1],
            *(t[slot:slot + 1] for t in self._slot_params()),
            [req.draw()])[0]
        req.generated.append(nxt)
        self.positions[slot] = len(req.prompt)
        self.next_token[slot] = nxt
        if req.max_new <= 1:
            self._finish(slot)

    def _slot_params(self):
        """The per-slot parameter tensors, uploaded again only after a
        slot changed owner."""
        if self._params_stale:
            torch = self._torch
            dev = self.device
            self._temp = torch.tensor(self._temp_host,
                                      dtype=torch.float32, device=dev)
            self._topk = torch.tensor(self._topk_host, dtype=torch.int32,
                                      device=dev)
            self._topp = torch.tensor(self._topp_host,
                                      dtype=torch.float32, device=dev)
            self._params_stale = False
        return self._temp, self._topk, self._topp

    # ------------------------------------------------------------- internals
    def _admit(self):
        torch = self._torch
        for slot in range(self.max_batch):
            if self.slots[slot] is not None or not self.queue:
                continue
            req = self.queue[0]
            if not self.cache.admit(slot, len(req.prompt) + req.max_new):
                return  # FIFO: nobody overtakes the waiting head
            self.queue.popleft()
            assert len(req.prompt) + req.max_new <= self.max_len, \
                "request longer than the slot capacity"
            self.slots[slot] = req
            if self.prefill_chunk is not None:
                # chunked: cache nothing yet; step() feeds chunks
                self._views[slot] = self.cache.slot_view(slot)
                self._prefill_done[slot] = 0
                self.positions[slot] = 0
                continue
            prompt = torch.tensor([req.prompt], device=self.device)
            view = self.cache.slot_view(slot)
            self.cache.ensure(slot, len(req.prompt))
            self.cache.sync()
            with torch.no_grad():
                logits = self.model(prompt, cache=view)
            self._first_token(slot, logits)

    def _prefill_step(self):
        """Advance every mid-prefill slot by one prompt chunk; a slot
        whose final chunk just ran emits its first token and joins the
        decode batch next step."""
        torch = self._torch
        for slot in range(self.max_batch):
            view = self._views[slot]
            if view is None:
                continue
            req = self.slots[slot]
            a = self._prefill_done[slot]
            b = min(a + self.prefill_chunk, len(req.prompt))
            chunk = torch.tensor([req.prompt[a:b]], device=self.device)
            self.cache.ensure(slot, b)
            self.cache.sync()
            with torch.no_grad():
                logits = self.model(chunk, cache=view)
            self._prefill_done[slot] = b
            if b < len(req.prompt):
                continue
            self._views[slot] = None
            self._first_token(slot, logits)

    def _finish(self, slot):
        self.cache.release(slot)
        self.slots[slot].done = True
        self.slots[slot] = None
        self.positions[slot] = 0
        self._views[slot] = None
        self._prefill_done[slot] = 0
        self._temp_host[slot] = 0.0
        self._params_stale = True

    def step(self):
        """Admit waiting requests, advance mid-prefill slots by one
        chunk, then decode one token for every active slot in a single
        batched pass. Returns the number of active slots decoded."""
        torch = self._torch
        self._admit()
        if self.prefill_chunk is not None:
            self._prefill_step()
        active = [i for i, r in enumerate(self.slots) if r is not None
                  and self._views[i] is None]
        if not active:
            return 0
        # every slot starts at the cache's idle position for the rows it
        # has cached: _prefill_done for a mid-prefill slot, and 0 for a
        # free one (_finish resets _prefill_done along with positions).
        # A decoding slot gets the page of the row it is about to write
        pos_list = [self.cache.idle_position(n)
                    for n in self._prefill_done]
        for i in active:
            self.cache.ensure(i, self.positions[i] + 1)
            pos_list[i] = self.positions[i]
        self.cache.sync()
        # one upload each for the token and the u vector
        tok_list = [0] * self.max_batch
        u_list = [0.0] * self.max_batch
        for i in active:
            tok_list[i] = self.next_token[i]
            u_list[i] = self.slots[i].draw()
        tokens = torch.tensor(tok_list, dtype=torch.long,
                              device=self.device).view(-1, 1)
        logits = self._decode(tokens, pos_list)
        ids = self._sample(logits[:, -1], *self._slot_params(), u_list)
        for i in active:
            req = self.slots[i]
            nxt = ids[i]
            req.generated.append(nxt)
            self.positions[i] += 1
            self.next_token[i] = nxt
            if len(req.generated) >= req.max_new:
                self._finish(i)
        return len(active)

    def run(self):
        """Drain the queue; returns {request_id: generated tokens}."""
        results = {}
        pending = list(self.queue)
        while self.queue or any(r is not None for r in self.slots):
            self.step()
        for req in pending:
            results[req.id] = req.generated
        return results
