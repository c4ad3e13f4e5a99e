"""The paged key/value cache's format in plain torch and its host bookkeeping (include/omnibiote_hip_paged.h): the tests' yardstick for the
paged kernels of csrc/attention_decode.hip, as kvquant.py is for the e4m3 format, and the two host objects that decide where things go —
``PageBook`` (which page holds which 64 positions of which row, and how many rows name it), ``PrefixIndex`` (which page holds which prompt
content) and ``PagedSchedule`` (which request runs in which slot, and when).  No
kernel is called here and nothing needs a GPU; ``generation.PagedKVCache`` adds the buffers to a ``PageBook`` and
``OmniBioTA.generate_many`` drives a ``PagedSchedule``.

One layer's pool: K bf16 [n_pages, H, 64, hs], V behind it in the same shape.  The table: int32 [rows, table_ld], entry j of row b the
page that holds positions [64 j, 64 j + 64) of that row; an entry outside [0, n_pages) means no page: nothing is stored there, and its
keys are not there.

The e4m3 pool (include/omnibiote_hip_paged8.h): K codes uint8 [n_pages, H, 64, hs], V codes, K scales fp32 [n_pages, H, 64], V scales, under
the same table; a head vector is quantised as ``kvquant.quantize_reference`` quantises it (``paged8_gather_reference``,
``paged8_scatter_reference``)."""
from __future__ import annotations

import torch

KV_PAGE = 64   # OBTE_KV_PAGE


def pages_for(n_positions: int) -> int:
    """the pages that cover ``n_positions`` positions"""
    return (int(n_positions) + KV_PAGE - 1) // KV_PAGE


def pool_bytes(n_pages, H, hs) -> int:
    """obte_kv_paged_bytes for a supported shape"""
    return 2 * n_pages * H * KV_PAGE * hs * 2


def paged_gather_reference(pool, table, n_pages, H, hs, T=None, fill=0.0):
    """The rectangular K and V a pool and a table stand for: (K, V), each bf16 [B, H, T, hs] with T = 64 * table_ld unless given (then
    the first T positions).  ``pool``: one layer's flat bf16 buffer; ``table``: int32 [B, table_ld] on any device.  The positions of an
    entry outside [0, n_pages) hold ``fill``.  Ordinary torch indexing, bit for bit a copy."""
    if pool.dtype != torch.bfloat16 or pool.numel() * 2 != pool_bytes(n_pages, H, hs):
        raise ValueError(f"paged_gather_reference: the pool must be {pool_bytes(n_pages, H, hs) // 2} bf16 values, got {pool.numel()} {pool.dtype}")
    if table.dim() != 2:
        raise ValueError(f"paged_gather_reference: the table must be (rows, table_ld), got {tuple(table.shape)}")
    B, ld = table.shape
    kv = pool.view(2, n_pages, H, KV_PAGE, hs)
    t = table.to(device=pool.device, dtype=torch.int64)
    there = (t >= 0) & (t < n_pages)
    # [2, B, ld, H, 64, hs] -> [2, B, H, ld * 64, hs]
    got = kv[:, torch.where(there, t, torch.zeros_like(t))]
    got = torch.where(there.view(1, B, ld, 1, 1, 1), got, torch.full_like(got, fill))
    rect = got.permute(0, 1, 3, 2, 4, 5).reshape(2, B, H, ld * KV_PAGE, hs)
    if T is not None:
        rect = rect[:, :, :, :T]
    return rect[0].contiguous(), rect[1].contiguous()


def paged_scatter_reference(K, V, table, n_pages, fill=float("nan")):
    """The inverse, for building a test's pool: K, V bf16 [B, H, T, hs] with T a multiple of 64 -> the flat pool in which page
    table[b][j] holds positions [64 j, 64 j + 64) of row b, and every page no entry names holds ``fill``."""
    B, H, T, hs = K.shape
    if T % KV_PAGE != 0 or table.shape != (B, T // KV_PAGE):
        raise ValueError(f"paged_scatter_reference: T = {T} must be a multiple of 64 and the table ({B}, {T // KV_PAGE}), got {tuple(table.shape)}")
    pool = torch.full((2, n_pages, H, KV_PAGE, hs), fill, dtype=torch.bfloat16, device=K.device)
    t = table.to(device=K.device, dtype=torch.int64)
    there = (t >= 0) & (t < n_pages)
    src = torch.stack([K, V]).view(2, B, H, T // KV_PAGE, KV_PAGE, hs).permute(0, 1, 3, 2, 4, 5)   # [2, B, ld, H, 64, hs]
    pool[:, t[there]] = src[:, there]
    return pool.view(-1)


def pool8_bytes(n_pages, H, hs) -> int:
    """obte_kv8_paged_bytes for a supported shape"""
    return 2 * n_pages * H * KV_PAGE * (hs + 4)


def _pool8_views(pool, n_pages, H, hs):
    """the codes [2, n_pages, H, 64, hs] (uint8) and the scales [2, n_pages, H, 64] (fp32) of one layer's flat uint8 e4m3 pool, as views"""
    n_codes = 2 * n_pages * H * KV_PAGE * hs
    return pool[:n_codes].view(2, n_pages, H, KV_PAGE, hs), pool[n_codes:].view(torch.float32).view(2, n_pages, H, KV_PAGE)


def paged8_gather_reference(pool, table, n_pages, H, hs, T=None, fill_code=0, fill_scale=0.0):
    """The rectangular codes and scales an e4m3 pool and a table stand for: (codes, scales), uint8 [2, B, H, T, hs] and fp32 [2, B, H, T]
    (index 0: K, 1: V; what the four regions of ``kvquant``'s rectangular cache hold), T = 64 * table_ld unless given (then the first T
    positions).  ``pool``: one layer's flat uint8 buffer; ``table``: int32 [B, table_ld] on any device.  The positions of an entry outside
    [0, n_pages) hold ``fill_code`` and ``fill_scale``.  Ordinary torch indexing, bit for bit a copy."""
    if pool.dtype != torch.uint8 or pool.numel() != pool8_bytes(n_pages, H, hs):
        raise ValueError(f"paged8_gather_reference: the pool must be {pool8_bytes(n_pages, H, hs)} uint8 values, got {pool.numel()} {pool.dtype}")
    if table.dim() != 2:
        raise ValueError(f"paged8_gather_reference: the table must be (rows, table_ld), got {tuple(table.shape)}")
    B, ld = table.shape
    codes, scales = _pool8_views(pool, n_pages, H, hs)
    t = table.to(device=pool.device, dtype=torch.int64)
    there = (t >= 0) & (t < n_pages)
    at = torch.where(there, t, torch.zeros_like(t))
    c = codes[:, at]                                                    # [2, B, ld, H, 64, hs]
    c = torch.where(there.view(1, B, ld, 1, 1, 1), c, torch.full_like(c, fill_code))
    s = scales[:, at]                                                   # [2, B, ld, H, 64]
    s = torch.where(there.view(1, B, ld, 1, 1), s, torch.full_like(s, fill_scale))
    c = c.permute(0, 1, 3, 2, 4, 5).reshape(2, B, H, ld * KV_PAGE, hs)
    s = s.permute(0, 1, 3, 2, 4).reshape(2, B, H, ld * KV_PAGE)
    if T is not None:
        c, s = c[:, :, :, :T], s[:, :, :, :T]
    return c.contiguous(), s.contiguous()


def paged8_scatter_reference(codes, scales, table, n_pages, fill_code=0x7F, fill_scale=float("nan")):
    """The inverse, for building a test's pool: codes uint8 [2, B, H, T, hs] and scales fp32 [2, B, H, T] with T a multiple of 64 -> the
    flat uint8 pool in which page table[b][j] holds positions [64 j, 64 j + 64) of row b, and every page no entry names holds the NaN
    code ``fill_code`` and ``fill_scale``."""
    two, B, H, T, hs = codes.shape
    if two != 2 or scales.shape != (2, B, H, T) or codes.dtype != torch.uint8 or scales.dtype != torch.float32:
        raise ValueError(f"paged8_scatter_reference: codes uint8 [2, B, H, T, hs] and scales fp32 [2, B, H, T], got {tuple(codes.shape)} and {tuple(scales.shape)}")
    if T % KV_PAGE != 0 or table.shape != (B, T // KV_PAGE):
        raise ValueError(f"paged8_scatter_reference: T = {T} must be a multiple of 64 and the table ({B}, {T // KV_PAGE}), got {tuple(table.shape)}")
    pool = torch.empty(pool8_bytes(n_pages, H, hs), dtype=torch.uint8, device=codes.device)
    pc, ps = _pool8_views(pool, n_pages, H, hs)
    pc.fill_(fill_code); ps.fill_(fill_scale)
    t = table.to(device=codes.device, dtype=torch.int64)
    there = (t >= 0) & (t < n_pages)
    pc[:, t[there]] = codes.view(2, B, H, T // KV_PAGE, KV_PAGE, hs).permute(0, 1, 3, 2, 4, 5)[:, there]   # from [2, B, ld, H, 64, hs]
    ps[:, t[there]] = scales.view(2, B, H, T // KV_PAGE, KV_PAGE).permute(0, 1, 3, 2, 4)[:, there]         # from [2, B, ld, H, 64]
    return pool


class PageBook:
    """Which page of a pool of ``n_pages`` holds which 64 positions of which of ``batch`` rows: the free list, the table as a CPU int32
    tensor (batch, ceil(max_len / 64)), -1 where there is no page, and an exact mirror of every row's position, -1 for a parked row.
    Host integers and one CPU tensor, no buffer and no device: ``PagedKVCache`` keeps the device copies in step with it.

    ``free_order`` (a sequence holding every page once): the order in which pages are handed out, first entry first; the default is
    0, 1, 2, ...  A released row's pages go to the back of the list.

    Pages may be SHARED between rows (``assign_shared``): ``refs[p]`` counts the rows whose table names page p, ``release`` lowers the
    counts and only a page that reaches zero goes back to the free list.  A page on the free list keeps its content until it is handed out
    again — ``on_hand_out(page)``, when set, is called at that moment (``PrefixIndex`` forgets the page there) — and ``assign_shared`` may
    name such a page: it is taken off the list again (revived).  With nothing shared every count is 0 or 1 and nothing here differs
    from a book without counts."""

    def __init__(self, batch, n_pages, max_len, free_order=None):
        self.batch, self.n_pages, self.max_len = int(batch), int(n_pages), int(max_len)
        if self.batch < 1 or self.n_pages < 1 or self.max_len < 1:
            raise ValueError(f"PageBook: batch, n_pages and max_len must be at least 1, got {batch}, {n_pages} and {max_len}")
        order = list(range(self.n_pages)) if free_order is None else [int(p) for p in free_order]
        if sorted(order) != list(range(self.n_pages)):
            raise ValueError(f"PageBook: free_order must hold every page of [0, {self.n_pages}) once")
        self.free = order
        self.table_ld = pages_for(self.max_len)
        self.table = torch.full((self.batch, self.table_ld), -1, dtype=torch.int32)
        self.row_pos = [-1] * self.batch          # the mirror: row b's next position, -1: parked
        self.row_pages = [[] for _ in range(self.batch)]
        self.refs = [0] * self.n_pages            # the rows that name each page
        self.on_hand_out = None                   # callable(page): the page leaves the free list for new content

    @property
    def pages_in_use(self):
        return self.n_pages - len(self.free)

    @property
    def max_row_pos(self):
        """the largest mirrored position (-1: every row is parked)"""
        return max(self.row_pos)

    def _row(self, row):
        row = int(row)
        if not 0 <= row < self.batch:
            raise ValueError(f"PageBook: row {row} outside [0, {self.batch})")
        return row

    def assign(self, row, n_positions):
        """Row ``row`` gets the pages that cover ``n_positions`` positions (it keeps the ones it has).  ValueError, with nothing changed,
        when the free list cannot cover them or they exceed ``max_len``.  Returns the pages added."""
        row, n_positions = self._row(row), int(n_positions)
        if not 0 <= n_positions <= self.max_len:
            raise ValueError(f"PageBook.assign: {n_positions} positions outside [0, max_len = {self.max_len}]")
        have = self.row_pages[row]
        more = pages_for(n_positions) - len(have)
        if more > len(self.free):
            raise ValueError(f"PageBook.assign: row {row} needs {more} more pages for {n_positions} positions and {len(self.free)} of {self.n_pages} are free")
        added = [self.free.pop(0) for _ in range(max(more, 0))]
        for p in added:
            if self.on_hand_out is not None:
                self.on_hand_out(p)
            self.refs[p] = 1
            self.table[row, len(have)] = p
            have.append(p)
        return added

    def check_shared(self, row, pages):
        """what ``assign_shared`` refuses, as a ValueError with nothing changed; returns (row, pages) as ints"""
        row = self._row(row)
        pages = [int(p) for p in pages]
        if self.row_pages[row]:
            raise ValueError(f"PageBook.assign_shared: row {row} still holds {len(self.row_pages[row])} pages (release it first)")
        if len(pages) > self.table_ld or len(set(pages)) != len(pages):
            raise ValueError(f"PageBook.assign_shared: row {row}: at most {self.table_ld} distinct pages, got {pages}")
        for p in pages:
            if not 0 <= p < self.n_pages:
                raise ValueError(f"PageBook.assign_shared: page {p} outside the pool's [0, {self.n_pages})")
        return row, pages

    def assign_shared(self, row, pages):
        """Row ``row``, which must hold no page, names ``pages`` in its first ``len(pages)`` table entries; each page's count goes up by
        one.  A named page that is on the free list is taken off it: a released page whose content is still valid is revived (nothing is
        told to ``on_hand_out``: the content stays).  ValueError with nothing changed for a row that holds pages or a page outside the
        pool.  Returns the pages revived."""
        row, pages = self.check_shared(row, pages)
        revived = [p for p in pages if self.refs[p] == 0]
        for p in revived:
            self.free.remove(p)
        for j, p in enumerate(pages):
            self.refs[p] += 1
            self.table[row, j] = p
        self.row_pages[row] = list(pages)
        return revived

    def place(self, row, position):
        """the mirror's writer: row ``row`` stands at ``position`` (-1: parked)"""
        self.row_pos[self._row(row)] = int(position)

    def release(self, row):
        """Row ``row`` gives its pages back, its table entries are cleared and it is parked.  A page another row still names stays in
        use; the others go to the back of the free list.  Returns the pages that did."""
        row = self._row(row)
        held, self.row_pages[row] = self.row_pages[row], []
        pages = []
        for p in held:
            self.refs[p] -= 1
            if self.refs[p] == 0:
                pages.append(p)
        self.free.extend(pages)
        self.table[row].fill_(-1)
        self.row_pos[row] = -1
        return pages

    def park_rows(self, rows):
        """the rows stop where they are (they keep their pages until released)"""
        for r in rows:
            self.row_pos[self._row(r)] = -1

    def grow_for_step(self):
        """Before a decode step: every active row whose position opens a new page gets one.  ValueError, with nothing changed, when the
        free list cannot serve them all or a row stands at ``max_len``.  Returns the rows whose table row changed."""
        need = [b for b, p in enumerate(self.row_pos) if p >= 0 and pages_for(p + 1) > len(self.row_pages[b])]
        full = [b for b, p in enumerate(self.row_pos) if p >= self.max_len]
        if full:
            raise ValueError(f"PageBook: rows {full} stand at the cache's last position ({self.max_len})")
        want = sum(pages_for(self.row_pos[b] + 1) - len(self.row_pages[b]) for b in need)
        if want > len(self.free):
            raise ValueError(f"PageBook: the step opens {want} new pages (rows {need}) and {len(self.free)} of {self.n_pages} are free")
        for b in need:
            self.assign(b, self.row_pos[b] + 1)
        return need

    def step(self):
        """after a decode step: every active row has one more position"""
        self.row_pos = [p + 1 if p >= 0 else p for p in self.row_pos]


class PrefixIndex:
    """Which page of a pool holds which 64 prompt tokens behind which earlier ones: what lets a request reuse the pages another request
    has filled.  A node is one page; its key is (the node of the page before it — 0 at position 0 —, the page's 64 tokens as a tuple), so a
    match compares the exact token content of whole pages, chained from position 0, and never a bare hash.  Pure host, no tensors.

    ``register(tokens, pages)`` records the ``len(tokens) // 64`` pages that prompt tokens cover completely, ``pages[j]`` holding tokens
    [64 j, 64 j + 64) (a chain that is recorded already keeps its page).  ``lookup(tokens)`` returns the longest recorded chain of pages
    for ``tokens``, at most ``(len(tokens) - 1) // 64`` of them: at least one token is always left to compute, because the first new token
    needs logits.  ``forget(page)`` drops a page; a chain through it ends before it (what lay behind becomes unreachable, and is dropped as
    its own pages are forgotten).  With ``book`` given the index makes itself the book's ``on_hand_out``: a page leaves the index when the
    ``PageBook`` hands it out again from the free list, so a released page stays findable for as long as the free list keeps it — first
    in, first out keeps it longest."""

    def __init__(self, book=None):
        self.nodes = {}        # (parent node, 64 tokens) -> (node, page)
        self.key_of = {}       # page -> its key
        self.next_node = 1     # (0: the root)
        if book is not None:
            book.on_hand_out = self.forget

    @staticmethod
    def _tokens(tokens):
        return [int(t) for t in (tokens.tolist() if isinstance(tokens, torch.Tensor) else tokens)]

    def register(self, tokens, pages):
        tokens = self._tokens(tokens)
        full = len(tokens) // KV_PAGE
        if len(pages) < full:
            raise ValueError(f"PrefixIndex.register: {len(tokens)} tokens cover {full} pages and {len(pages)} are given")
        parent = 0
        for j in range(full):
            key = (parent, tuple(tokens[KV_PAGE * j:KV_PAGE * j + KV_PAGE]))
            if key not in self.nodes:
                page = int(pages[j])
                self.forget(page)                                      # (a page holds one content)
                self.nodes[key] = (self.next_node, page)
                self.key_of[page] = key
                self.next_node += 1
            parent = self.nodes[key][0]

    def lookup(self, tokens):
        tokens = self._tokens(tokens)
        parent, pages = 0, []
        for j in range((len(tokens) - 1) // KV_PAGE if tokens else 0):
            hit = self.nodes.get((parent, tuple(tokens[KV_PAGE * j:KV_PAGE * j + KV_PAGE])))
            if hit is None:
                break
            parent = hit[0]
            pages.append(hit[1])
        return pages

    def forget(self, page):
        key = self.key_of.pop(int(page), None)
        if key is not None:
            del self.nodes[key]

    def __len__(self):
        return len(self.nodes)


class PagedSchedule:
    """Continuous batching as a pure host object, no tensors: ``lengths[r]`` prompt tokens and up to ``max_new_tokens`` new ones per
    request, ``batch`` slots, a pool of ``n_pages`` pages.  The rule (``OmniBioTA.generate_many``): requests wait in the given order; request r
    NEEDS ceil((lengths[r] + max_new_tokens) / 64) pages, all promised to it when it is admitted; it is admitted when a slot is free and
    the pages not promised to running requests cover its need; admission is strictly first-in first-out, nothing is skipped; a finished
    request gives slot and promise back at once.  ``n_pages=None``: ``batch`` times the largest need.  ValueError here, before anything
    runs: a request that can never fit (``lengths[r] + max_new_tokens > block_size``, or a need above ``n_pages``), an empty prompt.

    ``admit()`` returns the (request, slot) pairs that start now, lowest free slot first; ``finish(request)`` ends one; ``done`` once
    every request has finished.  Which pages a request holds is the cache's business (``PageBook``): the promise guarantees that its free
    list never runs dry."""

    def __init__(self, lengths, max_new_tokens, batch, n_pages=None, block_size=None):
        self.lengths = [int(n) for n in lengths]
        self.max_new, self.batch = int(max_new_tokens), int(batch)
        if self.batch < 1:
            raise ValueError(f"generate_many: batch must be at least 1, got {batch}")
        if self.max_new < 1:
            raise ValueError(f"generate_many: max_new_tokens must be at least 1, got {max_new_tokens}")
        if self.lengths and min(self.lengths) < 1:
            raise ValueError("generate_many: a prompt is empty")
        if block_size is not None:
            for r, n in enumerate(self.lengths):
                if n + self.max_new > block_size:
                    raise ValueError(f"generate_many: request {r}: {n} prompt tokens + {self.max_new} new ones exceed block_size = {block_size}")
        self.need = [pages_for(n + self.max_new) for n in self.lengths]
        largest = max(self.need, default=1)
        self.n_pages = self.batch * largest if n_pages is None else int(n_pages)
        for r, n in enumerate(self.need):
            if n > self.n_pages:
                raise ValueError(f"generate_many: request {r} needs {n} pages ({self.lengths[r]} prompt tokens + {self.max_new} new ones) and the pool has "
                                 f"n_pages = {self.n_pages}")
        self.next = 0                              # the first request still waiting
        self.slot_of = {}                          # running request -> slot
        self.free_slots = list(range(self.batch))
        self.promised = 0                          # pages promised to running requests
        self.finished = 0

    @property
    def done(self):
        return self.finished == len(self.lengths)

    def admit(self):
        """the requests that start now, in order: [(request, slot), ...] (empty: the head of the queue has to wait, or nothing waits)"""
        out = []
        while self.next < len(self.lengths) and self.free_slots and self.promised + self.need[self.next] <= self.n_pages:
            r, slot = self.next, self.free_slots.pop(0)
            self.slot_of[r] = slot
            self.promised += self.need[r]
            self.next += 1
            out.append((r, slot))
        return out

    def finish(self, request):
        """request ``request`` has ended: its slot and its promise are free again.  Returns the slot."""
        slot = self.slot_of.pop(request)
        self.free_slots.append(slot)
        self.free_slots.sort()
        self.promised -= self.need[request]
        self.finished += 1
        return slot
