"""Guard bands around device buffers: a plain helper module of the fenced tests (tests/test_hip_fenced.py, tests/test_fenced_host.py).

fenced() puts a payload into a larger buffer that is poison everywhere else: 16 bytes in front, so that the payload starts on a 16-byte
boundary and on nothing coarser (view.data_ptr() % 512 == 16), `ld - cols` columns behind every row when a leading dimension is asked
for, and a back guard taller than any tile of the library.  assert_guards() finds every byte a kernel wrote outside the payload;
poison that is NaN finds every read that reaches a result (assert_finite_where / assert_same_bits against the same call on plain
tensors)."""
import torch

NAN_BF16 = 0x7FC0                 # inputs: a read past the payload that reaches a result makes it NaN
NAN_F32 = 0x7FC00000
MARK = {1: 0x5A, 2: 0x1234, 4: 0x12341234, 8: 0x1234123412341234}   # outputs, integers: a pattern no kernel produces by accident
BACK_ROWS = 256                   # the tallest tile in the library
BACK_ELEMS = 4096                 # behind a 1-D buffer
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def poison_for(dtype, kind):
    """kind "nan": the quiet NaN of a floating dtype (the marker for an integer dtype); "mark": the marker pattern"""
    size = torch.empty((), dtype=dtype).element_size()
    if kind == "nan" and dtype == torch.bfloat16:
        return NAN_BF16
    if kind == "nan" and dtype == torch.float32:
        return NAN_F32
    assert kind in ("nan", "mark"), kind
    return MARK[size]


def filled(shape, dtype, poison="mark", device="cuda"):
    """a plain stand-alone tensor whose every element is the bit pattern `poison` ("nan", "mark" or an integer)"""
    size = torch.empty((), dtype=dtype).element_size()
    pat = poison_for(dtype, poison) if isinstance(poison, str) else int(poison)
    t = torch.empty(tuple(shape), dtype=_INT[size], device=device)
    t.fill_(pat if pat < 2 ** (8 * size - 1) or size == 1 else pat - 2 ** (8 * size))
    return t.view(dtype) if dtype != _INT[size] else t


class Fence:
    """keeps the whole buffer alive and knows where the payload lies in it"""

    def __init__(self, whole, first, rows, cols, ld, poison, view):
        self.whole, self.first, self.rows, self.cols, self.ld, self.poison, self.view = whole, first, rows, cols, ld, poison, view

    def outside_payload_not_poison(self):
        bad = self.whole != self.poison
        if self.rows * self.ld:
            bad[self.first:self.first + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        return bad


def fenced(t_or_shape, dtype=None, poison="mark", front_bytes=16, back_rows=BACK_ROWS, ld=None, device="cuda", fill=None):
    """(view, handle).  t_or_shape: a tensor (its values are copied in; dtype defaults to its own) or a shape.  The last dimension is
    the row, the others are flattened into rows; ld (elements, >= the row length) leaves ld - cols poisoned columns behind every
    row, the view is then strided.  poison: "nan", "mark" or an integer pattern of the element's size.  fill: a pattern written over
    the payload of a buffer without a tensor (default: it stays poison).  back_rows rows of ld elements follow the payload, at least
    4096 elements."""
    src = t_or_shape if torch.is_tensor(t_or_shape) else None
    shape = tuple(src.shape) if src is not None else tuple(int(v) for v in t_or_shape)
    dtype = dtype or src.dtype
    size = torch.empty((), dtype=dtype).element_size()
    pat = poison_for(dtype, poison) if isinstance(poison, str) else int(poison)
    cols = shape[-1] if shape else 1
    rows = 1
    for v in shape[:-1]:
        rows *= v
    ld = cols if ld is None else int(ld)
    assert ld >= cols and front_bytes % 16 == 0 and front_bytes > 0
    first = front_bytes // size
    back = max(back_rows * ld, BACK_ELEMS)
    n = first + rows * ld + back
    raw = torch.empty(n * size + 512, dtype=torch.uint8, device=device)
    skip = (-raw.data_ptr()) % 512
    whole = raw[skip:skip + n * size].view(_INT[size])
    whole.fill_(pat if pat < 2 ** (8 * size - 1) or size == 1 else pat - 2 ** (8 * size))
    pat = whole[0].item()
    typed = whole.view(dtype) if dtype != _INT[size] else whole
    if ld == cols:
        view = typed[first:first + rows * cols].view(shape)
    else:
        assert len(shape) >= 2, "a leading dimension needs rows"
        view = typed[first:first + rows * ld].view(rows, ld)[:, :cols]
        view = view if len(shape) == 2 else view.unflatten(0, shape[:-1])
    if src is not None:
        view.copy_(src.to(dtype))
    elif fill is not None:
        whole[first:first + rows * ld].view(rows, ld)[:, :cols].fill_(fill)
    assert view.data_ptr() % 512 == front_bytes % 512 and tuple(view.shape) == shape
    h = Fence(whole, first, rows, cols, ld, pat, view)
    h.raw = raw
    return view, h


def assert_guards(*handles):
    """every byte outside the payloads still holds the poison"""
    for h in handles:
        bad = h.outside_payload_not_poison()
        if bad.any():
            at = bad.nonzero().flatten()
            e0 = int(at[0]) - h.first
            where = f"{-e0} elements in front of the payload" if e0 < 0 else f"row {e0 // h.ld}, column {e0 % h.ld} (payload {h.rows} x {h.cols}, ld {h.ld})"
            raise AssertionError(f"guard overwritten: {at.numel()} elements, the first at {where}")


def _bits(t):
    t = t.contiguous()
    return t if not t.dtype.is_floating_point else t.view(_INT[t.element_size()])


def assert_finite_where(got, plain, what=""):
    """(b): finite wherever the plain call's output is finite"""
    if got.dtype.is_floating_point:
        bad = torch.isfinite(plain) & ~torch.isfinite(got)
        assert not bad.any(), f"{what}: {int(bad.sum())} values are not finite where the plain call's are"


def assert_same_bits(got, plain, what=""):
    """(b) and (c): bit for bit the plain call's output"""
    assert got.shape == plain.shape and got.dtype == plain.dtype, (what, got.shape, plain.shape)
    assert_finite_where(got, plain, what)
    diff = _bits(got) != _bits(plain)
    assert not diff.any(), f"{what}: {int(diff.sum())}/{diff.numel()} elements differ from the plain call, the first at {tuple(int(v) for v in diff.nonzero()[0])}"
