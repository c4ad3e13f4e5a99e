"""Host-side tests (no GPU) of the forward-only block path: the workspace size of obte_block_fwd_infer, its argument checks,
and the plan table's answer for the activation-only GELU epilogue (OBTE_EPI_GELU_ACT)."""
import pytest

from omnibiote_amd import _lib

EINVAL = -1


@pytest.mark.parametrize("B,T,C,H", [(2, 128, 128, 2), (8, 1024, 1024, 8), (32, 1024, 2048, 16)])
def test_infer_workspace_is_bounded_and_smaller_than_the_activation_buffer(B, T, C, H):
    lib = _lib.lib()
    n = lib.obte_block_infer_ws_bytes(B, T, C, H)
    assert 0 < n <= 8 * B * T * C * 2 + 4096, n
    assert n < lib.obte_block_act_bytes_p(B, T, C, H, 0.0)


def test_infer_workspace_is_zero_for_a_shape_the_block_rejects():
    lib = _lib.lib()
    assert lib.obte_block_infer_ws_bytes(2, 128, 128, 4) == 0      # head size 32
    assert lib.obte_block_infer_ws_bytes(2, 128, 8192, 64) == 0    # n_embd beyond 4096
    assert lib.obte_block_infer_ws_bytes(0, 128, 128, 2) == 0
    assert lib.obte_block_infer_ws_bytes(2, 128, 130, 2) == 0


def test_block_fwd_infer_rejects_a_null_descriptor():
    lib = _lib.lib()
    assert lib.obte_block_fwd_infer(None, 4096, 4096, 4096, 1 << 30, None) == EINVAL
    msg = lib.obte_last_error().decode()
    assert "obte_block_fwd_infer" in msg and "null" in msg, msg


def test_plan_table_takes_the_activation_only_epilogue_in_its_one_layout():
    lib = _lib.lib()
    try:
        assert _lib.EPI_GELU_ACT == 9
        assert lib.obte_gemm_plan_set(1, 1, _lib.EPI_GELU_ACT, 4096, 4096, 256, 7, 256, 1) == 0
        for structure, width in ((1, 128), (2, 128), (2, 192), (2, 256), (3, 256), (4, 128)):
            assert lib.obte_gemm_plan_set(1, 1, _lib.EPI_GELU_ACT, 512, 512, 256, structure, width, 1) == 0, (structure, width)
        assert lib.obte_gemm_plan_set(0, 0, _lib.EPI_GELU_ACT, 4096, 4096, 256, 7, 256, 1) == EINVAL
        assert lib.obte_last_error().decode().startswith("obte_gemm_plan_set")
        assert lib.obte_gemm_plan_set(1, 0, _lib.EPI_GELU_ACT, 512, 512, 256, 2, 256, 1) == EINVAL    # the dy W layout has no GELU
        assert lib.obte_gemm_plan_set(1, 1, _lib.EPI_GELU_ACT, 512, 512, 2048, 2, 256, 2) == EINVAL   # no split-K
        assert lib.obte_gemm_plan_set(1, 1, _lib.EPI_GELU_ACT, 512, 512, 256, 3, 128, 1) == EINVAL    # structure 3 is 256 wide
    finally:
        _lib.check(lib.obte_gemm_plan_clear(), "obte_gemm_plan_clear")


def test_abi_version_and_symbols_are_append_only():
    assert _lib.lib().obte_abi_version() == 1
    assert "obte_block_infer_ws_bytes" in _lib.SYMBOLS and "obte_block_fwd_infer" in _lib.SYMBOLS
