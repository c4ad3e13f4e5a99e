"""Host side of the step prelude's C entry points (include/omnibiote_hip.h: obte_key_ranges_from_tokens, obte_token_order,
obte_token_order_ws_bytes): every argument is validated on the host before any launch, so the rejections need no GPU — a
pointer that is merely non-null is enough, because no rejected call launches anything."""
import pytest

from omnibiote_amd import _lib

EINVAL = -1
P = 4096          # a non-null "pointer": rejected calls never dereference it


def _rejected(rc, *words):
    assert rc == EINVAL, rc
    msg = _lib.lib().obte_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_key_ranges_rejects_bad_arguments():
    f = _lib.lib().obte_key_ranges_from_tokens
    _rejected(f(None, 2, 8, 3, 0, 0, P, None), "obte_key_ranges_from_tokens", "null")
    _rejected(f(P, 2, 8, 3, 0, 0, None, None), "obte_key_ranges_from_tokens", "null")
    for B, T in ((0, 8), (-1, 8), (2, 0), (2, -5), (2, 1 << 24), (1 << 31, 8)):
        _rejected(f(P, B, T, 3, 0, 0, P, None), "obte_key_ranges_from_tokens", "shape")
    _rejected(f(P, 2, 8, 3, 1, -1, P, None), "obte_key_ranges_from_tokens", "group")


def test_token_order_rejects_bad_arguments():
    f = _lib.lib().obte_token_order
    for ids, order, ws in ((None, P, P), (P, None, P), (P, P, None)):
        _rejected(f(ids, 4, 64, 256, order, ws, None), "obte_token_order", "null")
    for segments, seg_len in ((0, 64), (-3, 64), (4, 0), (4, -1)):
        _rejected(f(P, segments, seg_len, 256, P, P, None), "obte_token_order", "shape")
    for vocab in (0, -7, (1 << 17) + 1, 1 << 20):
        _rejected(f(P, 4, 64, vocab, P, P, None), "obte_token_order", "vocab")
    for segments, seg_len in ((1, 1 << 31), (1 << 31, 1), (1 << 16, 1 << 15), (3, 1 << 30), (1 << 40, 1 << 40)):
        _rejected(f(P, segments, seg_len, 65536, P, P, None), "obte_token_order", "2^31")


def test_token_order_ws_bytes_is_positive_and_monotone():
    f = _lib.lib().obte_token_order_ws_bytes
    for vocab in (1, 8, 256, 257, 65536, 1 << 17):
        prev = 0
        for n in (1, 63, 64, 65, 1000, 1024, 1025, 32768, 100003, 1 << 20, (1 << 31) - 1):
            b = f(1, n, vocab)
            assert b > 0 and b >= prev, (vocab, n, b, prev)
            prev = b
        prev = 0
        for segments in (1, 2, 4, 7, 64, 1000):
            b = f(segments, 32768, vocab)
            assert b > 0 and b >= prev, (vocab, segments, b, prev)
            prev = b
    # more sorted bytes never need less room
    assert f(4, 32768, 8) <= f(4, 32768, 65536) <= f(4, 32768, 1 << 17)
    # a shape obte_token_order rejects has no size
    for segments, seg_len, vocab in ((0, 64, 256), (4, 0, 256), (4, 64, 0), (4, 64, (1 << 17) + 1), (1 << 16, 1 << 15, 256)):
        assert f(segments, seg_len, vocab) == 0
