"""CPU self-test of tests/fenced.py (no GPU): the guard bands and the three assertions of tests/test_hip_fenced.py bite.  The "kernels"
are torch functions on CPU buffers: one writes an element past its output, one reads the poisoned neighbour of its input into its
result, one stays in bounds."""
import pytest
import torch

from fenced import BACK_ELEMS, MARK, NAN_BF16, assert_finite_where, assert_guards, assert_same_bits, fenced

BF = torch.bfloat16


def _x(rows, cols):
    return (torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) % 13 - 6).to(BF)


def _flat(view, h, n):
    """the `n` elements of the buffer that start at the payload: what a kernel sees through the payload's pointer"""
    typed = h.whole.view(view.dtype) if view.dtype != h.whole.dtype else h.whole
    return typed[h.first:h.first + n]


@pytest.mark.parametrize("dtype,poison,size", [(BF, "nan", 2), (torch.float32, "nan", 4), (BF, "mark", 2), (torch.float32, "mark", 4),
                                               (torch.int32, "mark", 4), (torch.int64, "mark", 8), (torch.uint8, "mark", 1)])
def test_layout_and_poison(dtype, poison, size):
    src = torch.arange(5 * 24).reshape(5, 24).to(dtype)
    for ld in (None, 32):
        v, h = fenced(src, poison=poison, ld=ld, device="cpu")
        assert v.data_ptr() % 512 == 16 and torch.equal(v, src) and v.is_contiguous() == (ld is None)
        assert v.stride(0) == (ld or 24) and h.whole.numel() >= 16 // size + 5 * (ld or 24) + 256 * (ld or 24)
        assert_guards(h)
        outside = h.whole[h.first + 5 * (ld or 24):]
        if ld:
            assert (h.whole[h.first:h.first + 5 * ld].view(5, ld)[:, 24:] == h.poison).all()
        if poison == "nan":
            assert torch.isnan(outside.view(dtype)).all()
        else:
            assert (outside == MARK[size]).all()
        assert (h.whole[:h.first] == h.poison).all() and (h.whole[h.first + 5 * (ld or 24):] == h.poison).all()
    v, h = fenced((7,), dtype, poison, device="cpu")
    assert v.shape == (7,) and h.whole.numel() >= 7 + BACK_ELEMS and (h.whole == h.poison).all()
    v, h = fenced((2, 3, 8), dtype, poison, device="cpu", fill=0)
    assert v.shape == (2, 3, 8) and (v == 0).all()
    assert_guards(h)


def test_a_store_past_the_payload_is_found():
    x = _x(5, 24)
    for ld in (None, 32):
        for at in ("behind", "pad", "front"):
            out, h = fenced((5, 24), BF, "mark", ld=ld, device="cpu")
            out.copy_(x * 2)
            assert_guards(h)
            flat = _flat(out, h, 5 * (ld or 24) + 1)
            if at == "behind":
                flat[5 * (ld or 24)] = 1.0                       # one element past the last row
            elif at == "pad":
                if ld is None:
                    continue
                flat[24] = 1.0                                   # column 24 of row 0: between the rows
            else:
                h.whole[h.first - 1] = 0                         # one element in front
            with pytest.raises(AssertionError, match="guard overwritten"):
                assert_guards(h)


def test_a_store_far_behind_the_payload_is_found():
    out, h = fenced((3, 8), BF, "mark", device="cpu")
    out.zero_()
    h.whole[-1] = 0
    with pytest.raises(AssertionError, match="guard overwritten"):
        assert_guards(h)


def _row_sums_reading(n_read):
    """a fake kernel: the sum of every row of a [rows, 24] input, the LAST row summed over n_read elements from its start"""
    def kernel(view, flat):
        out = view.float().sum(1)
        out[-1] = flat[(view.shape[0] - 1) * view.stride(0):][:n_read].float().sum()
        return out
    return kernel


def test_a_read_of_the_poisoned_neighbour_is_found_and_an_in_bounds_kernel_passes():
    x = _x(5, 24)
    plain = _row_sums_reading(24)(x, x.flatten())
    for ld in (None, 32):
        v, h = fenced(x, poison="nan", ld=ld, device="cpu")
        flat = _flat(v, h, 5 * (ld or 24) + 8)
        good = _row_sums_reading(24)(v, flat)
        assert_guards(h)
        assert_finite_where(good, plain)
        assert_same_bits(good, plain)
        bad = _row_sums_reading(25)(v, flat)                     # one element past the row: NaN
        with pytest.raises(AssertionError, match="not finite"):
            assert_finite_where(bad, plain)
        with pytest.raises(AssertionError):
            assert_same_bits(bad, plain)
    # a finite neighbour (poison 1.0) still changes bits: (c) alone finds it
    v, h = fenced(x, poison=0x3F80, device="cpu")
    bad = _row_sums_reading(25)(v, _flat(v, h, 5 * 24 + 8))
    assert_finite_where(bad, plain)
    with pytest.raises(AssertionError, match="differ"):
        assert_same_bits(bad, plain)
    assert NAN_BF16 == 0x7FC0
